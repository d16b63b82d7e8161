"""Single-image / folder super-resolution with an RRDBNet, MSRResNet or RCAN checkpoint, denoising with a RIDNet one, or licence-
plate restoration with a GFPGANv1OCR one (the model the reference's inference.py:28-40 and its API scripts serve), on the HIP
path.

The SR / denoising archs keep the reference's I/O convention: read BGR uint8, /255, BGR->RGB CHW float
(img2tensor, img_util.py:9-35), network, clamp to [0,1], RGB->BGR HWC, *255 round (tensor2img, img_util.py:38-94 with
min_max=(0,1) as sr_model.py:148).  Large frames go through the tiler (tiling.py).

GFPGANv1OCR (--arch GFPGANv1OCR, scale 1, fp32, no tiling): the image is resized bilinearly (align_corners=False, no antialias;
exact cv2 parity is not claimed) to the network's input size, mapped to [-1, 1] (the training convention, mean / std 0.5; the
reference's inference.py feeds [0, 1], a quirk not reproduced), restored with return_rgb=False, converted with
tensor2img(min_max=(-1, 1)) and resized back to the input's size (inference.py:75).  The stored noise buffers are used, so the
output is reproducible; --randomize_noise draws fresh noise per call as the reference's scripts do.  The defaults are the
square product configuration of api_plate_oto.py / api1.py (256 x 256, num_style_feat 256, channel_multiplier 0.5, num_mlp 8,
input_is_latent, different_w, sft_half).

    python -m image_restoration_amd.inference --input crop.png --output out.png --model_path net_g.pth \
        [--num_block 23 --num_feat 64 --tile 512 --tile_pad 16 --compute_dtype fp32|bf16 --niqe_params niqe_pris_params.npz]
    python -m image_restoration_amd.inference --arch MSRResNet --scale 3 --input crop.png --output out.png --model_path net_g.pth
    python -m image_restoration_amd.inference --arch RCAN --scale 4 --input crop.png --output out.png --model_path RCAN_BIX4-official.pth
    python -m image_restoration_amd.inference --arch RIDNet --input noisy.png --output clean.png --model_path RIDNet.pth
    python -m image_restoration_amd.inference --arch GFPGANv1OCR --input plate.png --output restored.png --model_path net_g.pth \
        [--input_width 256 --input_height 256 --num_style_feat 256 --channel_multiplier 0.5 --num_mlp 8 --randomize_noise]
    python -m torch.distributed.run --nproc-per-node 8 -m image_restoration_amd.inference --launcher pytorch --tile 512 ...
"""
import argparse
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from .archs import build_network
from . import watchdog
from .tiling import tiled_forward
from .metrics.niqe import load_niqe_params, niqe_device
from .utils.img_util import img2tensor, tensor2img


def imread_bgr(path):
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def imwrite_bgr(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)


ARCH_DEFAULT_BLOCKS = {'RRDBNet': 23, 'MSRResNet': 16, 'RCAN': 20, 'RIDNet': 4}


def generator_options(args):
    """network_g option block of the command line.  RRDBNet: scale 1/2/4, fp32 or bf16; MSRResNet: upscale 2/3/4, fp32 only;
    RCAN: upscale 2/3/4/8, fp32 only, 20 blocks per group by default (the released checkpoints' layout); RIDNet: scale 1 (a
    denoiser), fp32 only, 4 EAMs by default, --num_feat = mid_channels."""
    arch = getattr(args, 'arch', 'RRDBNet')
    if arch == 'GFPGANv1OCR':
        if args.scale != 1:
            raise ValueError(f'--arch GFPGANv1OCR restores at the input size: it takes --scale 1 only, not {args.scale}')
        if getattr(args, 'compute_dtype', 'fp32') != 'fp32':
            raise ValueError('--arch GFPGANv1OCR runs in fp32 only (no --compute_dtype bf16)')
        if getattr(args, 'tile', 0):
            raise ValueError('--arch GFPGANv1OCR restores the whole image at the network size: no --tile')
        h, w = args.input_height, args.input_width
        if h < 8 or h & (h - 1) or w < h or w % h:
            raise ValueError(f'--arch GFPGANv1OCR needs --input_height a power of two >= 8 and --input_width a multiple of it, '
                             f'got {w} x {h}')
        return dict(type='GFPGANv1OCR', input_width=args.input_width, input_height=args.input_height,
                    num_style_feat=args.num_style_feat, channel_multiplier=args.channel_multiplier, narrow=args.narrow,
                    num_mlp=args.num_mlp, input_is_latent=True, different_w=True, sft_half=True)
    num_block = getattr(args, 'num_block', None)
    num_block = ARCH_DEFAULT_BLOCKS[arch] if num_block is None else num_block
    if arch == 'RIDNet':
        if args.scale != 1:
            raise ValueError(f'--arch RIDNet is a denoiser: it takes --scale 1 only, not {args.scale}')
        if getattr(args, 'compute_dtype', 'fp32') != 'fp32':
            raise ValueError('--arch RIDNet runs in fp32 only (no --compute_dtype bf16)')
        return dict(type='RIDNet', in_channels=3, mid_channels=args.num_feat, out_channels=3, num_block=num_block)
    if arch == 'RCAN':
        if args.scale not in (2, 3, 4, 8):
            raise ValueError(f'--arch RCAN takes --scale 2, 3, 4 or 8, not {args.scale}')
        if getattr(args, 'compute_dtype', 'fp32') != 'fp32':
            raise ValueError('--arch RCAN runs in fp32 only (no --compute_dtype bf16)')
        return dict(type='RCAN', num_in_ch=3, num_out_ch=3, num_feat=args.num_feat, num_group=getattr(args, 'num_group', 10),
                    num_block=num_block, squeeze_factor=getattr(args, 'squeeze_factor', 16), upscale=args.scale)
    if arch == 'MSRResNet':
        if args.scale not in (2, 3, 4):
            raise ValueError(f'--arch MSRResNet takes --scale 2, 3 or 4, not {args.scale}')
        if getattr(args, 'compute_dtype', 'fp32') != 'fp32':
            raise ValueError('--arch MSRResNet runs in fp32 only (no --compute_dtype bf16)')
        return dict(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=args.num_feat, num_block=num_block, upscale=args.scale)
    return dict(type='RRDBNet', num_in_ch=3, num_out_ch=3, scale=args.scale, num_feat=args.num_feat, num_block=num_block,
                num_grow_ch=args.num_grow_ch, compute_dtype=getattr(args, 'compute_dtype', 'fp32'))


def load_generator(args, device):
    if not args.model_path:
        torch.manual_seed(0)  # no checkpoint: every rank of a sharded run must still hold the same (random) weights
    net = build_network(generator_options(args))
    if args.model_path:
        from .utils.checkpoint import load_generator_weights
        load_generator_weights(net, args.model_path, strict=True)  # BasicSR files and official ESRGAN key names
    return net.to(device).eval()


def restore(net, img_bgr_u8, tile=0, tile_pad=16, scale=4, rank=0, world_size=1):
    """uint8 BGR image -> uint8 BGR x`scale` image.  With world_size > 1 (one process per GPU, every rank calls this with the
    same image) the tiles are sharded over the ranks and the result is assembled on rank 0 (None elsewhere)."""
    y = restore_tensor(net, img_bgr_u8, tile, tile_pad, scale, rank, world_size)
    return None if y is None else tensor2img(y, rgb2bgr=True, min_max=(0, 1))


def restore_tensor(net, img_bgr_u8, tile=0, tile_pad=16, scale=4, rank=0, world_size=1):
    """restore() before tensor2img: the [1, 3, H, W] RGB float output on the device (None off rank 0)."""
    x = img2tensor(img_bgr_u8.astype(np.float32) / 255., bgr2rgb=True, float32=True).unsqueeze(0).to(next(net.parameters()).device)
    with torch.no_grad():
        if tile and (max(x.shape[2:]) > tile or world_size > 1):
            y = tiled_forward(net, x, tile, tile_pad, scale, rank=rank, world_size=world_size)
        else:
            y = watchdog.guarded(lambda: net(x), 'restore') if rank == 0 else None   # tiled_forward guards itself
    return y


def gfpgan_restore(net, img_bgr_u8, randomize_noise=False):
    """uint8 BGR image -> uint8 BGR image of the same size through a GFPGANv1OCR: bilinear resize to the network's size, [0, 1] ->
    [-1, 1], forward with return_rgb=False, tensor2img(min_max=(-1, 1)), bilinear resize back (module docstring)."""
    h, w = img_bgr_u8.shape[:2]
    x = img2tensor(img_bgr_u8.astype(np.float32) / 255., bgr2rgb=True, float32=True).unsqueeze(0)
    if (h, w) != (net.input_height, net.input_width):
        x = F.interpolate(x, size=(net.input_height, net.input_width), mode='bilinear', align_corners=False)
    x = (x * 2 - 1).to(next(net.parameters()).device)
    with torch.no_grad():
        y, _ = watchdog.guarded(lambda: net(x, return_rgb=False, randomize_noise=randomize_noise), 'restore')
    out = tensor2img(y, rgb2bgr=True, min_max=(-1, 1))
    if out.shape[:2] != (h, w):
        t = torch.from_numpy(out.astype(np.float32)).permute(2, 0, 1).unsqueeze(0)
        t = F.interpolate(t, size=(h, w), mode='bilinear', align_corners=False)
        out = np.ascontiguousarray(t[0].permute(1, 2, 0).round().clamp(0, 255).numpy().astype(np.uint8))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--input', required=True, help='image file or folder')
    ap.add_argument('--output', required=True, help='output file or folder')
    ap.add_argument('--model_path', default=None)
    ap.add_argument('--scale', type=int, default=None, help='default: 1 for RIDNet, 4 otherwise')
    ap.add_argument('--num_feat', type=int, default=64)
    ap.add_argument('--arch', choices=('RRDBNet', 'MSRResNet', 'RCAN', 'RIDNet', 'GFPGANv1OCR'), default='RRDBNet',
                    help='generator: RRDBNet (ESRGAN; --scale 1/2/4), MSRResNet (--scale 2/3/4, fp32), RCAN (--scale 2/3/4/8, fp32), '
                         'the RIDNet denoiser (--scale 1, fp32) or the GFPGANv1OCR plate restorer (--scale 1, fp32, no --tile)')
    ap.add_argument('--num_block', type=int, default=None,
                    help='default: 23 for RRDBNet, 16 for MSRResNet, 20 (blocks per residual group) for RCAN, 4 (EAMs) for RIDNet')
    ap.add_argument('--num_group', type=int, default=10, help='RCAN: residual groups')
    ap.add_argument('--squeeze_factor', type=int, default=16, help='RCAN: channel-attention squeeze factor')
    ap.add_argument('--num_grow_ch', type=int, default=32)
    ap.add_argument('--input_width', type=int, default=256, help='GFPGANv1OCR: network input width (a multiple of the height)')
    ap.add_argument('--input_height', type=int, default=256, help='GFPGANv1OCR: network input height (a power of two >= 8)')
    ap.add_argument('--num_style_feat', type=int, default=256, help='GFPGANv1OCR: style code width')
    ap.add_argument('--channel_multiplier', type=float, default=0.5, help='GFPGANv1OCR: channel multiplier of the 64+ levels')
    ap.add_argument('--narrow', type=float, default=1.0, help='GFPGANv1OCR: channel narrowing')
    ap.add_argument('--num_mlp', type=int, default=8, help='GFPGANv1OCR: style MLP depth (8 in api1.py / api_plate_oto.py)')
    ap.add_argument('--randomize_noise', action='store_true',
                    help='GFPGANv1OCR: fresh noise per image (the reference scripts\' default) instead of the stored noise buffers')
    ap.add_argument('--tile', type=int, default=0,
                    help='split frames larger than this into tiles (0: whole image).  RCAN and RIDNet: their channel attention '
                         'pools over each tile, so a tiled output differs from the whole-image one (RIDNet\'s receptive field '
                         'without the attention has a radius of about 50 pixels: --tile_pad 16 still leaves seams)')
    ap.add_argument('--tile_pad', type=int, default=16)
    ap.add_argument('--launcher', choices=('none', 'pytorch'), default='none',
                    help="pytorch: started by torch.distributed.run, one process per GPU; the tiles of every image (--tile) are "
                         "sharded over the ranks, rank 0 writes the results")
    ap.add_argument('--dist_backend', default='nccl', help='process-group backend of --launcher pytorch (nccl = RCCL)')
    ap.add_argument('--compute_dtype', choices=('fp32', 'bf16'), default='fp32',
                    help='fp32 = the reference arithmetic; bf16 = reduced-precision kernels (about 6x faster)')
    ap.add_argument('--niqe_params', default=None, metavar='PATH',
                    help="print the NIQE of each restored image (no reference needed; computed on the device); PATH is BasicSR's "
                         'niqe_pris_params.npz, the pristine model')
    args = ap.parse_args(argv)
    if args.scale is None:
        args.scale = 1 if args.arch in ('RIDNet', 'GFPGANv1OCR') else 4
    try:
        generator_options(args)
    except ValueError as e:
        ap.error(str(e))
    if args.arch == 'GFPGANv1OCR' and (args.niqe_params or args.launcher != 'none'):
        ap.error('--arch GFPGANv1OCR takes neither --niqe_params nor --launcher')
    rank, world = 0, 1
    if args.launcher == 'pytorch':
        from .utils.dist_util import get_dist_info, init_dist
        init_dist('pytorch', backend=args.dist_backend)
        rank, world = get_dist_info()
        if not args.tile:
            ap.error('--launcher pytorch shards tiles: give --tile')
    if args.niqe_params:
        load_niqe_params(args.niqe_params)  # a missing pristine model fails before any image is restored
    net = load_generator(args, torch.device('cuda'))
    paths = sorted(glob.glob(os.path.join(args.input, '*'))) if os.path.isdir(args.input) else [args.input]
    for p in paths:
        if args.arch == 'GFPGANv1OCR':
            out = gfpgan_restore(net, imread_bgr(p), args.randomize_noise)
            dst = os.path.join(args.output, os.path.basename(p)) if os.path.isdir(args.input) else args.output
            imwrite_bgr(dst, out)
            print(f'{p} -> {dst} {out.shape}')
            continue
        y = restore_tensor(net, imread_bgr(p), args.tile, args.tile_pad, args.scale, rank, world)
        if y is None:
            continue
        out = tensor2img(y, rgb2bgr=True, min_max=(0, 1))
        dst = os.path.join(args.output, os.path.basename(p)) if os.path.isdir(args.input) else args.output
        imwrite_bgr(dst, out)
        print(f'{p} -> {dst} {out.shape}')
        if args.niqe_params:
            print(f'{dst} NIQE {niqe_device(y, 0, args.niqe_params)[0]:.4f}')
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
