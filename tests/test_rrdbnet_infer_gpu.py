"""The RRDBNet inference (no_grad) forward on every route it can take: csrc/rrdbnet.hip forward_body / forward_impl and
csrc/rrdbnet_bf16.hip forward_h.  The training forward runs none of that code, and the rest of the suite reaches only the shipped
widths at sizes where the Winograd switch is all on or all off.

A. fp32, configuration x dispatch matrix against float64 (oracle/rrdbnet_ref.py on .double() tensors): widths where every conv,
   only the trunk and head, only conv1-4 of the blocks or nothing is eligible for conv_wino_f32, one to three 32-cout groups, cin
   chunk counts with every remainder mod 3, no blocks, pixel-unshuffled inputs, the CB8 + sr_cb8_to_nchw_f32 tail of num_out_ch > 4;
   shapes where the size rule (H*W >= 128*128 of ONE image's output map) takes some convs of a forward and not others.  Each case runs
   sr_dev_set_wino_f32 0, 1 and one forced tile variant and asserts
     1 the Winograd launches in the launch profile are those of the dispatch rule, restated here (wino_launches);
     2 max|y - y64| < 1e-4 (TOL of tests/test_rrdbnet_gpu.py);
     3 err_on <= 4 err_off + 2^-20 (tests/test_wino_f32_gpu.py: test_network_switch_on_against_switch_off has the derivation);
     4 a mode in which the rule gives no Winograd launch gives the bits of mode 0;
     5 a plain call gives the bits of the profiled one, image n-1 alone the bits of its slice of the batch;
     6 mode 0 gives the bits of the TRAINING forward: the same direct kernels on the same descriptors, four rotating concat buffers
       and the feat0 copy against one buffer per dense block.
B. Image groups (run_image_groups, shift_space, one sync block per group): fp32 with sr_dev_set_group_min_wgs(1) so that small maps
   split, 2 / 3 / 4 groups against one, bit for bit, on even and uneven splits, with the direct kernels, a forced Winograd variant
   and the chain launch (sr_set_conv_chain_f32(1)); bf16 at the smallest shapes its own rule groups,
   (n / groups) * ceil(w / 32) * ceil(h / 32) >= 64, under the fused dense block (sr_set_conv_chain 3, the default) and the chain
   launch (2, what the watchdog falls back to), and one image against oracle/bf16_sim.py (relative L2 1e-3, tests/fuzz/net_fuzz.py).

The launch profiler disables grouping (forward_impl: `groups <= 1 || prof_on()`) and the chain launch (sr_conv3x3_chain_f32:
`!sr::prof_on()`), so no profiled call is part of a grouped comparison, and that the chain launch is the one taken is read from its
hand-off words in the forward workspace instead: a launch that ran leaves its work counters above zero, a forward that went conv by
conv leaves the block as the forward's memset made it.

Every switch is restored by a fixture finalizer and in `finally`: wino 1, group_min_wgs 0 (= 512), forward_groups 0, chain_f32 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4                          # tests/test_rrdbnet_gpu.py
WINO_IDS = {2: 106, 3: 107, 4: 108}  # sr_dev_set_wino_f32(mode) -> kernel id of its tile variant
CHAIN_BF16_DEFAULT = 3              # conv_bf16.hip: g_chain_enabled
CHAIN_EPOCHS = 256                  # conv_bf16.hip SR_CHAIN_EPOCHS (kEpochs of sr_conv3x3_chain_f32): work counters per sync block


def _restore(lib):
    lib.sr_dev_set_wino_f32(1)
    lib.sr_dev_set_group_min_wgs(0)
    lib.sr_set_forward_groups(0)
    lib.sr_set_conv_chain_f32(0)


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_f32.restype = C.c_int
    lib.sr_dev_set_group_min_wgs.argtypes = [C.c_int]
    lib.sr_dev_set_group_min_wgs.restype = None
    yield lib
    _restore(lib)


@pytest.fixture(autouse=True)
def switches(lib):
    yield
    _restore(lib)


class nan_outputs:
    """Inside this block every fp32 tensor that torch.empty hands out starts as NaN.  RRDBNet._launch takes its output from
    torch.empty, and the caching allocator gives a block freed a moment ago, still holding an earlier call's (correct) output, to the
    next call of the same size: a forward that leaves part of its output unwritten would inherit the very values it is compared with.
    Seeded like this, whatever a forward does not write is NaN and fails every comparison."""

    def __enter__(self):
        self._empty = empty = torch.empty

        def seeded(*args, **kw):
            t = empty(*args, **kw)
            return t.fill_(float('nan')) if t.dtype == torch.float32 else t

        torch.empty = seeded
        return self

    def __exit__(self, *exc):
        torch.empty = self._empty
        return False


def _profiled(lib, fn):
    _lib.check(lib.sr_profile_start(1024), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 1024)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 1024, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i].kernel_id for i in range(min(cnt.value, 1024))]


def _cfg(num_in_ch, num_out_ch, scale, num_feat, num_grow_ch, num_block):
    return dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, scale=scale, num_feat=num_feat, num_block=num_block,
                num_grow_ch=num_grow_ch)


CONFIGS = {
    'all32': _cfg(3, 3, 4, 32, 32, 1),       # everything eligible; 4, 8, 12, 16, 20 cin chunks (remainders 1 and 2 mod 3); one cout group
    'wide': _cfg(3, 3, 4, 96, 64, 1),        # three and two 32-cout groups, up to 44 chunks
    'trunk_only': _cfg(3, 3, 4, 64, 16, 1),  # conv5 eligible, conv1 not: blocks direct, conv_body / up1 / up2 / hr Winograd
    'block_only': _cfg(3, 3, 4, 48, 32, 1),  # conv1-4 have Winograd images, conv5 and the trunk have none: no Winograd launch
    'head': _cfg(3, 3, 4, 64, 32, 0),        # no blocks: conv_body reads feat0 as source and as skip
    's2': _cfg(3, 3, 2, 32, 32, 1),          # pixel-unshuffled input, cin0 12, output 2x
    's1': _cfg(3, 3, 1, 32, 32, 1),          # cin0 48, output 1x
    'chans15': _cfg(1, 5, 4, 64, 32, 1),     # W.last + sr_cb8_to_nchw_f32 tail
    'chans41': _cfg(4, 1, 4, 32, 32, 1),     # one-channel NCHW tail
    'dflt': _cfg(3, 3, 4, 64, 32, 2),        # the shipped widths
    'bf16': _cfg(3, 3, 4, 64, 32, 1),        # the shipped widths at a one-block depth (B, bf16)
}
UNSHUFFLE = {4: 1, 2: 2, 1: 4}

# (n, h, w) of the feature map; the input is h * m x w * m with m the pixel_unshuffle factor
ODD = (3, 13, 37)
BY_SIZE = [(2, 32, 32),   # only conv_up2 and conv_hr reach 128 x 128
           (2, 24, 44),   # 96 x 176 = 16896 >= 16384: three 64-column tiles with a 48-column tail
           (1, 31, 33)]   # 124 x 132 = 16368 < 16384: nothing crosses
CASES = [(cid, ODD) for cid in ('all32', 'wide', 'trunk_only', 'block_only', 'head', 's2', 's1', 'chans15', 'chans41', 'dflt')]
CASES += [(cid, s) for cid in ('dflt', 'all32', 'trunk_only', 'chans15', 'chans41') for s in BY_SIZE]
CASES += [('dflt', (1, 64, 64))]  # conv_up1's output crosses too


def _case_id(case):
    cid, (n, h, w) = case
    return f'{cid}-{n}x{h}x{w}'


def wino_launches(cfg, h, w, mode):
    """The dispatch rule of forward_body, restated: the number of conv_wino_f32 launches of one forward over h x w feature maps.
    conv_first and conv_last never; a conv is eligible iff cout % 32 == 0 and cin >= 8; a block's five convs only if its conv1 and
    its conv5 are both eligible; mode 0 none, mode 1 those whose own output map has H * W >= 128 * 128, mode 2.. all eligible."""
    if mode == 0:
        return 0
    nf, gc, nb = cfg['num_feat'], cfg['num_grow_ch'], cfg['num_block']

    def eligible(cout, cin):
        return cout % 32 == 0 and cin >= 8

    def by_size(H, W):
        return mode >= 2 or H * W >= 128 * 128

    block = [(gc, nf + k * gc) for k in range(4)] + [(nf, nf + 4 * gc)]
    count = 0
    if eligible(*block[0]) and eligible(*block[4]) and by_size(h, w):
        count += 3 * nb * sum(eligible(*c) for c in block)
    for H, W in ((h, w), (2 * h, 2 * w), (4 * h, 4 * w), (4 * h, 4 * w)):  # conv_body, conv_up1, conv_up2, conv_hr
        count += int(eligible(nf, nf) and by_size(H, W))
    return count


_NETS = {}
_REFS = {}


def _net(cid, dev, dtype='fp32'):
    if (cid, dtype) not in _NETS:
        cfg = CONFIGS[cid]
        net = ira.build_network(dict(type='RRDBNet', compute_dtype=dtype, **cfg)).to(dev).eval()
        seed = list(CONFIGS).index(cid)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.rrdbnet_state_dict(seed, **cfg).items()}, strict=True)
        _NETS[(cid, dtype)] = net
    return _NETS[(cid, dtype)]


def _input(cid, shape):
    n, h, w = shape
    cfg = CONFIGS[cid]
    m = UNSHUFFLE[cfg['scale']]
    return synth.uniform_input(1000 + 7 * h + w, (n, cfg['num_in_ch'], h * m, w * m))


def reference(cid, shape):
    """(x, y64): float64 oracle output, computed once per (config, shape) and read-only."""
    if (cid, shape) not in _REFS:
        from oracle import rrdbnet_ref as R
        cfg = CONFIGS[cid]
        seed = list(CONFIGS).index(cid)
        sd = {k: torch.from_numpy(v).double() for k, v in synth.rrdbnet_state_dict(seed, **cfg).items()}
        x = _input(cid, shape)
        with torch.no_grad():
            y64 = R.rrdbnet_forward(torch.from_numpy(x).double(), sd, cfg['scale'], cfg['num_block']).numpy()
        x.setflags(write=False)
        y64.setflags(write=False)
        _REFS[(cid, shape)] = (x, y64)
    return _REFS[(cid, shape)]


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('idx', range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_fp32_configuration_dispatch_matrix_against_float64(cuda, lib, idx):
    cid, shape = CASES[idx]
    cfg, (n, h, w) = CONFIGS[cid], shape
    forced = (2, 3, 4)[idx % 3]
    x, y64 = reference(cid, shape)
    y64 = torch.from_numpy(y64.copy())
    net = _net(cid, cuda)
    xd = torch.from_numpy(x.copy()).to(cuda)

    def run(mode):
        lib.sr_dev_set_wino_f32(mode)
        with torch.no_grad():
            net(xd)  # packs the weights outside the profiled call
            box = []
            ids = _profiled(lib, lambda: box.append(net(xd)))
            y = net(xd)
            y_last = net(xd[n - 1:n])
        torch.cuda.synchronize()
        return y.cpu(), box[0].cpu(), y_last.cpu(), ids

    try:
        runs = {mode: run(mode) for mode in (0, 1, forced)}
        lib.sr_dev_set_wino_f32(0)
        y_train = net(xd.clone().requires_grad_()).detach().cpu()
    finally:
        _restore(lib)

    bad = []
    y_off = runs[0][0]
    err_off = float((y_off.double() - y64).abs().max())
    for mode, (y, y_prof, y_last, ids) in runs.items():
        expect = wino_launches(cfg, h, w, mode)
        if cid == 'block_only' or (mode == 1 and shape == (1, 31, 33)):
            assert expect == 0, 'the restated rule disagrees with the case table'
        got = sum(ids.count(k) for k in WINO_IDS.values())
        err = float((y.double() - y64).abs().max())
        print(f'{_case_id(CASES[idx])} mode {mode}: wino launches {got} (rule {expect}) err_off {err_off:.3e} err {err:.3e} '
              f'ratio {err / max(err_off, 1e-30):.3f}')
        if got != expect:
            bad.append(f'1 mode {mode}: {got} Winograd launches, the rule gives {expect}: {ids}')
        if mode >= 2 and ids.count(WINO_IDS[mode]) != got:
            bad.append(f'1 mode {mode}: a variant other than the forced one ran: {ids}')
        if not err < TOL:
            bad.append(f'2 mode {mode}: max|y - y64| = {err:.3e}')
        if not err <= 4 * err_off + 2.0 ** -20:
            bad.append(f'3 mode {mode}: err_on {err:.3e} > 4 * err_off {err_off:.3e} + 2^-20')
        if expect == 0 and not torch.equal(y, y_off):
            bad.append(f'4 mode {mode}: no Winograd launch, but not the bits of mode 0')
        if not torch.equal(y, y_prof):
            bad.append(f'5 mode {mode}: the plain call differs from the profiled call')
        if not torch.equal(y[n - 1:n], y_last):
            bad.append(f'5 mode {mode}: image {n - 1} alone differs from its slice of the batch')
        if not bool(torch.isfinite(y).all()):
            bad.append(f'2 mode {mode}: not finite')
    if not torch.equal(y_off, y_train):
        d = float((y_off.double() - y_train.double()).abs().max())
        bad.append(f'6 mode 0 differs from the training forward (max abs {d:.3e})')
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- B
GROUP_CASES = [(cid, n) for cid in ('dflt', 'chans15') for n in (5, 2, 1)]  # 4 groups of 5 images are 2, 1, 1, 1; of 2 images two; of 1 one


@pytest.mark.parametrize('idx', range(len(GROUP_CASES)), ids=[f'{c}-n{n}' for c, n in GROUP_CASES])
def test_fp32_image_groups_give_the_bits_of_one_group(cuda, lib, idx):
    """Every output starts as NaN (nan_outputs) and the one-group output stays alive on the device, so a group that writes another
    group's slice of y, or none, cannot pass: without the `n0 * out_img` offset of the grouped call the slices of the later images
    stay NaN."""
    cid, n = GROUP_CASES[idx]
    net = _net(cid, cuda)
    xd = torch.from_numpy(_input(cid, (n, 24, 40))).to(cuda)
    forced = (2, 3, 4)[idx % 3]
    bad = []
    try:
        lib.sr_dev_set_group_min_wgs(1)
        for mode in (0, forced):
            lib.sr_dev_set_wino_f32(mode)
            with torch.no_grad(), nan_outputs():
                _lib.check(lib.sr_set_forward_groups(1), 'sr_set_forward_groups')
                net(xd)
                y1 = net(xd)
                for g in (2, 3, 4):
                    _lib.check(lib.sr_set_forward_groups(g), 'sr_set_forward_groups')
                    yg = net(xd)
                    if not torch.equal(yg, y1):
                        bad.append(f'mode {mode}, {g} groups of {n} images: {int((yg != y1).sum())} elements differ, '
                                   f'{int(torch.isnan(yg).sum())} NaN')
                    del yg
            assert bool(torch.isfinite(y1).all())
    finally:
        _restore(lib)
    assert not bad, bad


def _handoff_words(lib, net, cfg, n, h, w):
    """The four sync blocks of the last forward's workspace as int32 [4][sync_ints].  This restates rrdbnet.hip's carve_fwd (the sync
    area is the LAST area of the workspace: kSyncBlocks = 4 blocks of sr_conv3x3_chain_sync_ints ints, rounded up to 256 bytes) and
    the block layout of sr_conv3x3_chain_sync_ints (conv_bf16.hip): [0] abort word, [1 + i] for i < CHAIN_EPOCHS the work counter
    of the i-th chain launch on the block, then one progress word per tile.  A layout change there has to be repeated here; the
    asserts below fail first if the sizes no longer fit."""
    ws = next(iter(net._workspaces.values()))
    nbytes = lib.sr_rrdbnet_workspace_bytes(C.byref(_lib.RRDBNetCfg(cfg['num_in_ch'], cfg['num_out_ch'], cfg['scale'], cfg['num_feat'],
                                                                    cfg['num_block'], cfg['num_grow_ch'])), n, h, w)
    ints = lib.sr_conv3x3_chain_sync_ints(n, h, w)
    area = (ints * 4 * 4 + 255) // 256 * 256
    assert ints > 1 + CHAIN_EPOCHS and 0 < area < nbytes <= ws.numel()
    return ws[nbytes - area:nbytes - area + ints * 16].view(torch.int32).view(4, ints).cpu()


def test_fp32_image_groups_on_the_chain_launch(cuda, lib):
    """sr_conv3x3_chain_f32 takes one launch per dense block when h % 16 == 0 and ceil(w / 32) * (h / 16) * n * (groups running side
    by side) >= 512.  With 5 images in groups of 2, 1, 1, 1 that is 128 tiles per image: 256 x 256, the smallest shape at which every
    group of the split takes it (tests/test_chain_f32_gpu.py: the same threshold on one stream).  The only place where two groups
    use different sync blocks of the hand-off words; the six dense blocks of a group share one."""
    from image_restoration_amd import watchdog
    cfg = CONFIGS['dflt']
    n, h, w = 5, 256, 256
    calls = 3 * cfg['num_block']
    net = _net('dflt', cuda)
    xd = torch.from_numpy(synth.uniform_input(41, (n, 3, h, w))).to(cuda)

    def run(chain, groups):
        _lib.check(lib.sr_set_conv_chain_f32(chain), 'sr_set_conv_chain_f32')
        _lib.check(lib.sr_set_forward_groups(groups), 'sr_set_forward_groups')
        with torch.no_grad(), nan_outputs():  # whatever a group does not write stays NaN
            y = net(xd)
        torch.cuda.synchronize()
        return y.cpu(), _handoff_words(lib, net, cfg, n, h, w)

    try:
        lib.sr_dev_set_wino_f32(0)
        lib.sr_dev_set_group_min_wgs(1)
        with torch.no_grad():
            net(xd)
        y_plain, words_plain = run(0, 1)
        y_one, words_one = run(1, 1)
        y_four, words_four = run(1, 4)
        watchdog.verify('test: fp32 chain launch in image groups')
    finally:
        _restore(lib)
    assert not bool(words_plain.any()), 'conv by conv, but hand-off words were written'
    for words in (words_one, words_four):
        assert not bool(words[:, 0].any()), 'a hand-off wait timed out'
    assert bool((words_one[0, 1:1 + calls] > 0).all()) and not bool(words_one[1:].any()), 'one group: six chain launches on sync block 0'
    assert bool((words_four[:, 1:1 + calls] > 0).all()), 'four groups: six chain launches on each of the four sync blocks'
    assert not bool(words_four[:, 1 + calls:1 + CHAIN_EPOCHS].any()), 'a work counter beyond the six chain launches of a group'

    assert torch.equal(y_one, y_plain), 'chain launch against conv by conv'
    assert torch.equal(y_four, y_one), 'four image groups against one, on the chain launch'
    assert bool(torch.isfinite(y_one).all())


def _bf16_input(n):
    return synth.uniform_input(77, (18, 3, 128, 128))[:n]


@pytest.mark.parametrize('n', [16, 18])  # four groups of four; 5, 5, 4, 4
def test_bf16_image_groups_give_the_bits_of_one_group(cuda, lib, n):
    """The benchmark's own inference conditions at a one-block depth: 128 x 128 images are 16 workgroups of 32 x 32, so four groups
    need 16 images.  Nothing here provokes a hand-off time-out; watchdog.verify turns one into a failure."""
    from image_restoration_amd import watchdog
    net = _net('bf16', cuda, 'bf16')
    xd = torch.from_numpy(_bf16_input(n)).to(cuda)
    bad = []
    try:
        for chain in (CHAIN_BF16_DEFAULT, 2):
            _lib.check(lib.sr_set_conv_chain(chain), 'sr_set_conv_chain')
            with torch.no_grad(), nan_outputs():  # y1 stays on the device; what a group does not write is NaN
                _lib.check(lib.sr_set_forward_groups(1), 'sr_set_forward_groups')
                net(xd)
                y1 = net(xd)
                for g in (0, 2, 3):
                    _lib.check(lib.sr_set_forward_groups(g), 'sr_set_forward_groups')
                    yg = net(xd)
                    if not torch.equal(yg, y1):
                        bad.append(f'chain {chain}: groups {g} of {n} images: {int((yg != y1).sum())} elements differ, '
                                   f'{int(torch.isnan(yg).sum())} NaN')
                    del yg
                for i in (0, n - 1):
                    if not torch.equal(net(xd[i:i + 1]), y1[i:i + 1]):
                        bad.append(f'chain {chain}: image {i} alone differs from its slice of the batch')
            watchdog.verify(f'test: bf16 image groups, sr_set_conv_chain({chain})')
            assert bool(torch.isfinite(y1).all())
    finally:
        lib.sr_set_conv_chain(2 if watchdog.fallback_count else CHAIN_BF16_DEFAULT)
        _restore(lib)
    assert not bad, bad


def test_bf16_single_image_against_the_bf16_storage_model(cuda, lib):
    """Image 0 of the grouped batches alone (the grouped test ties every batch slice to it bit for bit) against the float64 model of
    bf16 storage: relative L2 < 1e-3, the bound tests/fuzz/net_fuzz.py holds for the bf16 output."""
    from image_restoration_amd import watchdog
    from oracle.bf16_sim import rrdbnet_forward_bf16_storage
    cfg = CONFIGS['bf16']
    x = _bf16_input(1)
    seed = list(CONFIGS).index('bf16')
    sd = {k: torch.from_numpy(v).double() for k, v in synth.rrdbnet_state_dict(seed, **cfg).items()}
    with torch.no_grad():
        y64 = rrdbnet_forward_bf16_storage(torch.from_numpy(x).double(), sd, cfg['scale'], cfg['num_block'])
        y = _net('bf16', cuda, 'bf16')(torch.from_numpy(x).to(cuda)).cpu().double()
    watchdog.verify('test: bf16 single image')
    rel = float((y - y64).norm() / y64.norm())
    print(f'bf16 1x3x128x128 against the bf16 storage model: relative L2 {rel:.3e}')
    assert rel < 1e-3, rel
