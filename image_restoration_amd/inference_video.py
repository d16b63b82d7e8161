"""Restore a folder of frames with an EDVR checkpoint on the HIP path: one forward per centre frame over the clip of
``--num_frame`` frames around it.

I/O convention of inference.py: read BGR uint8, /255, BGR->RGB CHW float (img2tensor), network, clamp to [0, 1], RGB->BGR HWC,
*255 round (tensor2img with min_max=(0, 1)).  The frames are the image files of ``--input`` in sorted order; past either end of
the sequence the clip is filled by ``--padding`` (data_util.generate_frame_indices).  Every frame is padded by replication to the
network's size multiple (4; 16 with --hr_in) and the output is cropped back.  Each output PNG carries its input's name.

No per-frame feature cache (the feature extraction of a frame runs once per clip that contains it) and no tiling: the whole
frame goes through the network at once.

    python -m image_restoration_amd.inference_video --input FRAMES_DIR --output OUT_DIR --model_path net_g.pth \
        [--num_frame 5 --padding reflection --compute_dtype fp32|bf16 --num_feat 64 --deformable_groups 8 \
         --num_extract_block 5 --num_reconstruct_block 10 --center_frame_idx N --hr_in --with_predeblur --no_tsa]
"""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import watchdog
from .archs import build_network
from .data.data_util import generate_frame_indices
from .inference import imread_bgr, imwrite_bgr
from .utils.img_util import img2tensor, tensor2img

EXTENSIONS = ('.png', '.jpg', '.jpeg', '.bmp')


def edvr_options(args):
    """network_g option block of the command line."""
    return dict(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=args.num_feat, num_frame=args.num_frame,
                deformable_groups=args.deformable_groups, num_extract_block=args.num_extract_block,
                num_reconstruct_block=args.num_reconstruct_block, center_frame_idx=args.center_frame_idx, hr_in=args.hr_in,
                with_predeblur=args.with_predeblur, with_tsa=not args.no_tsa, compute_dtype=args.compute_dtype)


def load_edvr(args, device):
    if not args.model_path:
        torch.manual_seed(0)
    net = build_network(edvr_options(args))
    if args.model_path:
        from .utils.checkpoint import load_generator_weights
        load_generator_weights(net, args.model_path, strict=True)
    return net.to(device).eval()


def frame_paths(folder):
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(EXTENSIONS))
    if not names:
        raise ValueError(f'{folder}: no image files ({", ".join(EXTENSIONS)})')
    return [os.path.join(folder, n) for n in names]


def load_frames(paths):
    """[T, 3, H, W] RGB float in [0, 1] on the CPU; the frames must share one size."""
    frames = [img2tensor(imread_bgr(p).astype(np.float32) / 255., bgr2rgb=True, float32=True) for p in paths]
    if any(f.shape != frames[0].shape for f in frames):
        raise ValueError('the frames of a sequence must have one size')
    return torch.stack(frames)


def restore_clip(net, clip):
    """[t, 3, H, W] RGB float on the device -> the restored centre frame [1, 3, sH, sW] (s = 1 with hr_in, else 4): replication
    padding up to the network's size multiple, one forward, the crop."""
    t, c, h, w = clip.shape
    m, s = (16, 1) if net.hr_in else (4, 4)
    ph, pw = (-h) % m, (-w) % m
    if ph or pw:
        clip = F.pad(clip, (0, pw, 0, ph), mode='replicate')
    with torch.no_grad():
        y = watchdog.guarded(lambda: net(clip.unsqueeze(0).contiguous()), 'restore_clip')
    return y[:, :, :s * h, :s * w]


def restore_folder(net, in_dir, out_dir, padding='reflection'):
    """Restores every frame of ``in_dir`` into ``out_dir`` (PNG, the input's base name); returns the written paths."""
    paths = frame_paths(in_dir)
    device = next(net.parameters()).device
    frames = load_frames(paths).to(device)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for i, p in enumerate(paths):
        idx = generate_frame_indices(i, len(paths), net.num_frame, padding=padding)
        y = restore_clip(net, frames[idx])
        out = os.path.join(out_dir, os.path.splitext(os.path.basename(p))[0] + '.png')
        imwrite_bgr(out, tensor2img(y, rgb2bgr=True, min_max=(0, 1)))
        written.append(out)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--input', required=True, help='folder of frames')
    ap.add_argument('--output', required=True, help='output folder')
    ap.add_argument('--model_path', default=None)
    ap.add_argument('--num_frame', type=int, default=5)
    ap.add_argument('--padding', default='reflection', choices=['replicate', 'reflection', 'reflection_circle', 'circle'])
    ap.add_argument('--compute_dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--num_feat', type=int, default=64)
    ap.add_argument('--deformable_groups', type=int, default=8)
    ap.add_argument('--num_extract_block', type=int, default=5)
    ap.add_argument('--num_reconstruct_block', type=int, default=10)
    ap.add_argument('--center_frame_idx', type=int, default=None)
    ap.add_argument('--hr_in', action='store_true')
    ap.add_argument('--with_predeblur', action='store_true')
    ap.add_argument('--no_tsa', action='store_true')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('inference_video runs only on a HIP device (no CPU fallback)')
    net = load_edvr(args, torch.device('cuda:0'))
    written = restore_folder(net, args.input, args.output, args.padding)
    print(f'{len(written)} frames -> {args.output}')


if __name__ == '__main__':
    main()
