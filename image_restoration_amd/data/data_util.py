"""Which LQ file belongs to which GT file (behaviour of basicsr/data/data_util.py:108-231, golden G-s).

Three sources of pairs: two folders (LQ name = ``filename_tmpl.format(<GT stem>) + <GT extension>``), a meta-info file listing GT names,
or two LMDB directories with equal key sets.  All return ``[{'<lq key>_path': ..., '<gt key>_path': ...}, ...]``."""
import os


def scandir(folder):
    """Names of the regular, non-hidden files directly inside ``folder``, sorted (the reference walks in os.scandir order, which
    depends on the file system; sorting yields the same SET of pairs in a reproducible order)."""
    with os.scandir(folder) as it:
        return sorted(entry.name for entry in it if entry.is_file() and entry.name[:1] != '.')


def _two(seq, what):
    if len(seq) != 2:
        raise AssertionError(f'The len of {what} should be 2 with [input_{what[:-1]}, gt_{what[:-1]}]. But got {len(seq)}')
    return seq


def _lq_name(gt_name, filename_tmpl):
    stem, ext = os.path.splitext(os.path.basename(gt_name))
    return filename_tmpl.format(stem) + ext


def _pair(lq_key, gt_key, lq_value, gt_value):
    return {lq_key + '_path': lq_value, gt_key + '_path': gt_value}


def paired_paths_from_folder(folders, keys, filename_tmpl):
    lq_dir, gt_dir = _two(folders, 'folders')
    lq_key, gt_key = _two(keys, 'keys')
    lq_names, gt_names = scandir(lq_dir), scandir(gt_dir)
    if len(lq_names) != len(gt_names):
        raise AssertionError(f'{lq_key} and {gt_key} datasets have different number of images: {len(lq_names)}, {len(gt_names)}.')
    present = frozenset(lq_names)
    pairs = []
    for gt_name in gt_names:
        want = _lq_name(gt_name, filename_tmpl)
        if want not in present:
            raise AssertionError(f'{want} is not in {lq_key}_paths.')
        pairs.append(_pair(lq_key, gt_key, os.path.join(lq_dir, want), os.path.join(gt_dir, gt_name)))
    return pairs


def paired_paths_from_meta_info_file(folders, keys, meta_info_file, filename_tmpl):
    """Each non-empty line of the meta-info file starts with a GT file name (anything after the first blank is ignored)."""
    lq_dir, gt_dir = _two(folders, 'folders')
    lq_key, gt_key = _two(keys, 'keys')
    with open(meta_info_file) as f:
        listed = [ln.split(' ')[0] for ln in (raw.strip() for raw in f) if ln]
    return [_pair(lq_key, gt_key, os.path.join(lq_dir, _lq_name(n, filename_tmpl)), os.path.join(gt_dir, n)) for n in listed]


def lmdb_keys(folder):
    """Keys of an ``*.lmdb`` directory = the part before the first '.' of each ``meta_info.txt`` line (``name.png (h,w,c) level``)."""
    with open(os.path.join(folder, 'meta_info.txt')) as f:
        return [ln.split('.')[0] for ln in f]


def paired_paths_from_lmdb(folders, keys):
    lq_dir, gt_dir = _two(folders, 'folders')
    lq_key, gt_key = _two(keys, 'keys')
    if not (lq_dir.endswith('.lmdb') and gt_dir.endswith('.lmdb')):
        raise ValueError(f'{lq_key} folder and {gt_key} folder should both in lmdb formats. But received '
                         f'{lq_key}: {lq_dir}; {gt_key}: {gt_dir}')
    names = set(lmdb_keys(lq_dir))
    if names != set(lmdb_keys(gt_dir)):
        raise ValueError(f'Keys in {lq_key}_folder and {gt_key}_folder are different.')
    return [_pair(lq_key, gt_key, n, n) for n in sorted(names)]


_FRAME_PADDINGS = ('replicate', 'reflection', 'reflection_circle', 'circle')


def generate_frame_indices(crt_idx, max_frame_num, num_frames, padding='reflection'):
    """The ``num_frames`` frame numbers (from 0) of the clip centred on frame ``crt_idx`` of a sequence of ``max_frame_num``
    frames.  Where the window of ``num_frames // 2`` frames on either side reaches past an end of the sequence, ``padding``
    says which frame stands in for a position ``d`` frames past that end (d = 1 is the first missing frame):

        replicate          the end frame itself
        reflection         the frame d inside the end, mirrored at the end frame
        reflection_circle  the frame d beyond the window's other side, so the stand-ins continue the clip away from the end
        circle             the position shifted by ``num_frames`` back into the sequence

    With crt_idx = 0 and num_frames = 5 these give [0, 0, 0, 1, 2], [2, 1, 0, 1, 2], [4, 3, 0, 1, 2] and [3, 4, 0, 1, 2].
    An even ``num_frames`` or an unknown mode is a ValueError."""
    if num_frames % 2 != 1:
        raise ValueError(f'generate_frame_indices: num_frames={num_frames} must be odd (a clip has a centre frame)')
    if padding not in _FRAME_PADDINGS:
        raise ValueError(f'generate_frame_indices: unknown padding {padding!r}; one of {", ".join(_FRAME_PADDINGS)}')
    last, half = max_frame_num - 1, num_frames // 2
    first_pos, last_pos = crt_idx - half, crt_idx + half
    out = []
    for pos in range(first_pos, last_pos + 1):
        if 0 <= pos <= last:
            out.append(pos)
            continue
        before = pos < 0
        d = -pos if before else pos - last
        if padding == 'replicate':
            out.append(0 if before else last)
        elif padding == 'reflection':
            out.append(d if before else last - d)
        elif padding == 'reflection_circle':
            out.append(last_pos + d if before else first_pos - d)
        else:
            out.append(pos + num_frames if before else pos - num_frames)
    return out


def generate_gaussian_kernel(kernel_size=13, sigma=1.6):
    """The ``kernel_size`` x ``kernel_size`` Gaussian of ``duf_downsample`` (float64 numpy), in closed form: the outer product of
    the 1D Gaussian exp(-x^2 / (2 sigma^2)) truncated at radius int(4 sigma + 0.5) and normalised to sum 1 — what Gaussian
    smoothing of a unit impulse gives while the radius fits in the kernel, so that no boundary rule enters (sigma 0.8 / 1.2 / 1.6
    at 13 taps: radius 3 / 5 / 6).  A radius that does not fit is a ValueError."""
    import numpy as np
    radius = int(4.0 * float(sigma) + 0.5)
    if radius > kernel_size // 2:
        raise ValueError(f'generate_gaussian_kernel: sigma={sigma} needs radius {radius}, which does not fit in {kernel_size} taps')
    xs = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (float(sigma) * float(sigma)) * xs ** 2)
    g = g / g.sum()
    k1 = np.zeros(kernel_size)
    k1[kernel_size // 2 - radius:kernel_size // 2 + radius + 1] = g
    return np.outer(k1, k1)


def duf_downsample(x, kernel_size=13, scale=4):
    """The downsampling of the official DUF code on frames [b, t, c, h, w] (or [t, c, h, w]): reflect padding by
    ``kernel_size // 2 + 2 * scale``, the Gaussian of sigma ``0.4 * scale`` at stride ``scale``, then two rows and columns cut
    from every side.  Runs where ``x`` lies, in its dtype."""
    import torch
    from torch.nn import functional as F
    if scale not in (2, 3, 4):
        raise ValueError(f'Only support scale (2, 3, 4), but got {scale}.')
    squeeze = x.ndim == 4
    if squeeze:
        x = x.unsqueeze(0)
    b, t, c, h, w = x.size()
    pad = kernel_size // 2 + scale * 2
    x = F.pad(x.reshape(-1, 1, h, w), (pad, pad, pad, pad), 'reflect')
    kernel = torch.from_numpy(generate_gaussian_kernel(kernel_size, 0.4 * scale)).type_as(x).unsqueeze(0).unsqueeze(0)
    x = F.conv2d(x, kernel, stride=scale)[:, :, 2:-2, 2:-2]
    x = x.reshape(b, t, c, x.size(2), x.size(3))
    return x.squeeze(0) if squeeze else x
