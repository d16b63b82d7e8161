"""Data side of the path: the rank-aware sampler of the reference, the paired and LQ-only image datasets with the crop / flip
augmentation and prefetchers, the REDS training clips and the per-folder video test set, and synthetic paired /
clip datasets for benchmarks / smoke training."""
from .data_sampler import EnlargedSampler  # noqa: F401
from .paired_image_dataset import PairedImageDataset  # noqa: F401
from .device_pipeline import DeviceClipPipeline, DeviceDegradePipeline, DevicePatchPipeline  # noqa: F401
from .ocr_degradation_dataset import OCRDegradationDataset  # noqa: F401
from .prefetch_dataloader import (BackgroundIterator, CPUPrefetcher, CUDAPrefetcher, DeviceFeed, HostFeed,  # noqa: F401
                                  PrefetchDataLoader)
from .reds_dataset import REDSDataset, REDSRecurrentDataset  # noqa: F401
from .single_image_dataset import SingleImageDataset  # noqa: F401
from .synthetic_clip_dataset import SyntheticClipDataset  # noqa: F401
from .synthetic_dataset import SyntheticPairedDataset  # noqa: F401
from .video_test_dataset import VideoRecurrentTestDataset, VideoTestDataset, VideoTestDUFDataset  # noqa: F401
