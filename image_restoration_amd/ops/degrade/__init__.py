"""The tensor degradations of the reference (utils/img_process_util.py:filter2D, utils/diffjpeg.py:DiffJPEG,
data/degradations.py:*_pt) on libsr_hip.so (include/sr_hip_degrade.h)."""
from .degrade import (DiffJPEG, DiffJPEGFunction, add_gaussian_noise_pt, degrade_finish, filter2D, quality_to_factor,
                      random_add_gaussian_noise_pt, resize_bilinear)

__all__ = ['DiffJPEG', 'DiffJPEGFunction', 'add_gaussian_noise_pt', 'degrade_finish', 'filter2D', 'quality_to_factor',
           'random_add_gaussian_noise_pt', 'resize_bilinear']
