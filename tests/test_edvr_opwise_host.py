"""The references of tests/test_edvr_opwise_gpu.py checked without the code under test (no GPU).

  The per-op float64 references of tests/edvr_opwise.py, composed by the network's own layer list (``EDVR._run`` on the ops table
      ``Ref64Ops``), reproduce tests/edvr_restate.py in float64 for the three configurations.  At b = 2 the output agrees to the last bit, although
      the restatement aligns the frames one by one on batches of b images and the layer list aligns b * t at once.  At b = 1
      (predeblur-hr-b1) it agrees within 5.4e-13 (1.2e-13 of the largest value; asserted below 1e-11 of it): the restatement then calls
      its 128-channel 3x3 convs (the PCD convs on a concatenation) on ONE image, and torch's CPU float64 conv2d sums those 1152 products
      in another order for a batch of one than for a batch of three (measured op by op: those eight convs differ by up to 3e-14 between
      the two batch sizes, every other reference is the same for every batch size); the deformable convs that read the offsets carry
      the difference on.  The input gradient agrees to float64 rounding in all three.  With the slopes as the kernels hold them, float32(0.1)
      instead of 0.1, the composition moves by the relative 1.5e-8 of that constant: measured 0.8e-8 to 7.9e-8 of the output's largest value, asserted below 1e-6.
  The seeds: the first of 20 .. 29 that meets both conditions of tests/test_edvr_gpu.py in the float64 restatement.
  The deformable convolution's backward on a forced cell equals autograd of tests/dcn_restate.py wherever the float32 and the float64
      cell agree, and samples planted within float32 rounding of an integer coordinate do land in another cell.
  Every negative control of the GPU test differs from the true reference by more than twice the bound it is tested under, so a
      correct kernel cannot pass both.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
import edvr_opwise as O  # noqa: E402
from edvr_opwise import CONFIGS, EPS  # noqa: E402

_CASES = {}


def _case(name):
    """(net, sd, x, gy, float64 restatement's output and level-1 offsets, composed output, ops log), once per configuration."""
    if name not in _CASES:
        net, sd, x, gy = O.make_case(name)
        offs = {}
        y64 = O.restated(sd, x, None, CONFIGS[name][0], torch.float64, offs)
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            yc, ops = O.composed(net, x.double(), mp)
        _CASES[name] = dict(net=net, sd=sd, x=x, gy=gy, y64=y64, offs=offs, yc=yc, log=ops.log)
    return _CASES[name]


def _fp32(*ts):
    """The values rounded to float32, as float64: what a recorded op's inputs are."""
    return [t.detach().float().double() for t in ts]


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_composed_references_reproduce_the_restatement(name):
    c = _case(name)
    kw = CONFIGS[name][0]
    assert c['yc'].dtype == torch.float64 and c['yc'].shape == c['y64'].shape
    diff = float((c['yc'] - c['y64']).abs().max())
    print(f'{name}: composed per-op references against edvr_restate, max |difference| = {diff:.3e}')
    if c['x'].size(0) >= 2:
        assert torch.equal(c['yc'], c['y64'])
    else:   # b == 1: torch's float64 conv2d over 128 channels sums in another order for ONE image than for three (module docstring)
        assert diff <= 1e-11 * float(c['y64'].abs().max())
    # the gradient of the input through both, float64 autograd
    xa, xb = (c['x'].double().requires_grad_(True) for _ in range(2))
    with pytest.MonkeyPatch.context() as mp:
        ya, _ = O.composed(c['net'], xa, mp)
    ga, = torch.autograd.grad(ya, xa, c['gy'].double())
    p = {k: v.double() for k, v in c['sd'].items()}
    yb = O.E.edvr(p, xb, num_frame=kw['num_frame'], deformable_groups=kw['deformable_groups'], **O.BLOCKS, hr_in=kw.get('hr_in', False),
                  with_predeblur=kw.get('with_predeblur', False), with_tsa=kw.get('with_tsa', True))
    gb, = torch.autograd.grad(yb, xb, c['gy'].double())
    rel = float((ga - gb).norm() / gb.norm())
    print(f'{name}: input gradient, relative L2 difference = {rel:.3e}')
    assert rel <= 1e-11                # the same sums, taken over t in another order (expand against stack)
    # the slopes as the kernels hold them
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        y32, _ = O.composed(c['net'], c['x'].double(), mp, slope32=True)
    moved = float((y32 - c['y64']).abs().max() / c['y64'].abs().max())
    print(f'{name}: float32(0.1) slopes move the output by {moved:.3e} of its largest value')
    assert 0 < moved < 1e-6


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_seed_is_the_first_that_deforms(name):
    kw, _, _, seed = CONFIGS[name]
    for s in range(20, seed + 1):
        if s == seed:
            off = _case(name)['offs']['l1']
        else:
            _, sd, x, _ = O.make_case(name, s)
            offs = {}
            O.restated(sd, x, None, kw, torch.float64, offs)
            off = offs['l1']
        mean_l1, outside = O.deforms(off, kw['deformable_groups'])
        print(f'{name} seed {s}: mean |offset| at level 1 = {mean_l1:.3f} px, outside {100 * outside:.1f} %')
        assert (0.5 <= mean_l1 <= 3.0 and outside >= 0.01) == (s == seed)


def _dcn_inputs(entry):
    x, off, logit, pack, slope, dg = entry
    x, off, logit = _fp32(x, off, logit)
    return x, off, logit, pack.weight.detach().double(), pack.bias.detach().double(), slope, dg


def test_the_forced_cell_backward_is_autograd_where_the_cells_agree():
    entries = [e for op, e in _case('nf16-dg2-notsa')['log'] if op == 'dcn' and e[0].size(2) == 8]
    assert len(entries) == 2            # level 1 and the cascade, 8 x 12
    planted = 0
    for k, entry in enumerate(entries):
        x, off, logit, wt, b, _, dg = _dcn_inputs(entry)
        n, _, h, w = off.shape
        # within float32 rounding of an integer coordinate: base - 1e-9 is in cell base - 1 in float64 and IS base in float32 (base >=
        # 1); the sample's other coordinate is put at a quarter, inside the image
        for img, ch, yy, xx in ((0, 0, 4, 3), (n - 1, 18 + 9, 2, 7), (1, 5, 5, 1)):
            off[img, ch, yy, xx] = float(torch.tensor(-1e-9, dtype=torch.float32))
            off[img, ch ^ 1, yy, xx] = 0.25
        c32, c64 = O.cells32(off, dg), O.cells64(off, dg)
        differ = (c32[0] != c64[0]) | (c32[1] != c64[1]) | (c32[2] != c64[2])          # [n, dg, 9, h, w]
        planted += int(differ.sum())
        assert int(differ.sum()) >= 3, 'the planted samples change cell between float32 and float64'
        dz = torch.randn((n, wt.size(0), h, w), dtype=torch.float64, generator=torch.Generator().manual_seed(k))
        leaves = [t.clone().requires_grad_(True) for t in (x, off, logit, wt, b)]
        z = R.modulated_deform_conv(leaves[0], leaves[1], torch.sigmoid(leaves[2]), leaves[3], leaves[4], dg)
        auto = torch.autograd.grad(z, leaves, dz)
        same = O.dcn_backward(x, off, logit, wt, b, dg, dz, c64)
        for name, a, g in zip(('dx', 'doffset', 'dmask', 'dweight', 'dbias'), auto, same):
            assert torch.equal(a, g), f'dcn {k} {name}: on the float64 cell the forced reference is not autograd of the restatement'
        forced = O.dcn_backward(x, off, logit, wt, b, dg, dz, c32)
        agree_o = (~differ).unsqueeze(3).expand(n, dg, 9, 2, h, w).reshape(n, 18 * dg, h, w)
        agree_m = (~differ).reshape(n, 9 * dg, h, w)
        assert torch.equal(forced[1][agree_o], auto[1][agree_o]) and torch.equal(forced[2][agree_m], auto[2][agree_m])
        assert not torch.equal(forced[1][~agree_o], auto[1][~agree_o]), 'across the kink d/d(offset) takes the other cell'
        # the value itself is continuous: columns on either cell differ by rounding only
        m = torch.sigmoid(logit)
        assert float((O.columns_forced(x, off, m, dg, c32) - R.columns(x, off, m, dg)).abs().max()) <= 1e-6
    print(f'{planted} samples change cell')


def _miss(got_true, mutated):
    """Largest |mutated reference - true reference| / bound, the bound being the mutated reference's own (what the GPU test applies)."""
    want, bound = mutated
    return float(((want - got_true).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('control', ['dcn_offsets_swapped', 'dcn_mask_group_shifted', 'avg_pool_valid_count', 'up2_align_corners',
                                     'conv_s2_odd_positions', 'tsa_corr_other_clip', 'sum_over_t_one_frame', 'upconv_lrelu_slope'])
def test_every_negative_control_leaves_its_bound(control):
    ratios = {}
    if control in ('dcn_offsets_swapped', 'dcn_mask_group_shifted'):
        mutate = 'swap' if control == 'dcn_offsets_swapped' else 'mask_group'
        for name in ('tsa-b2', 'nf16-dg2-notsa'):
            for k, (op, entry) in enumerate(e for e in _case(name)['log'] if e[0] == 'dcn'):
                x, off, logit, wt, b, slope, dg = _dcn_inputs(entry)
                true = O.dcn_spec(x, off, logit, wt, b, slope, dg)['fwd'][0]
                ratios[f'{name} dcn {k}'] = _miss(true, O.dcn_spec(x, off, logit, wt, b, slope, dg, mutate=mutate)['fwd'])
        assert len(ratios) == 8
    elif control == 'avg_pool_valid_count':
        for k, (x,) in enumerate(e for op, e in _case('tsa-b2')['log'] if op == 'pool'):
            x, = _fp32(x)
            ratios[f'pool {k}'] = _miss(O.pool_spec(x)['fwd'][0], O.pool_spec(x, mutate='valid_count')['fwd'])
        assert len(ratios) == 2
    elif control == 'up2_align_corners':
        for name in CONFIGS:
            for k, (x,) in enumerate(e for op, e in _case(name)['log'] if op == 'up2'):
                x, = _fp32(x)
                ratios[f'{name} up2 {k}'] = _miss(O.up2_spec(x)['fwd'][0], O.up2_spec(x, mutate='align_corners')['fwd'])
        assert len(ratios) == 6 + 8 + 4
    elif control in ('conv_s2_odd_positions', 'upconv_lrelu_slope'):
        op, mutate = ('conv_s2', 'odd') if control == 'conv_s2_odd_positions' else ('conv', 'slope')
        for name in CONFIGS:
            net = _case(name)['net']
            for k, (x, m, slope) in enumerate(e for o, e in _case(name)['log'] if o == op):
                if mutate == 'slope' and m not in (net.upconv1, net.upconv2):
                    continue
                x, = _fp32(x)
                w, b = m.weight.detach().double(), m.bias.detach().double()
                stride = 2 if op == 'conv_s2' else 1
                ratios[f'{name} {op} {k}'] = _miss(O.conv_spec(x, w, b, slope, stride)['fwd'][0],
                                                   O.conv_spec(x, w, b, slope, stride, mutate=mutate)['fwd'])
        assert len(ratios) == (2 + 6 + 2 if op == 'conv_s2' else 6)
    elif control == 'tsa_corr_other_clip':
        (emb, ref, al, t), = [e for op, e in _case('tsa-b2')['log'] if op == 'tsa_corr']
        emb, ref, al = _fp32(emb, ref, al)
        ratios['tsa_corr'] = _miss(O.corr_spec(emb, ref, al, t)['fwd'][0], O.corr_spec(emb, ref, al, t, mutate='other_clip')['fwd'])
    else:
        # the production plumbing itself: the centre frame expanded over t, on leaves
        ops = O.Ref64Ops()
        for b, t in ((2, 3), (1, 3), (2, 5)):
            gen = torch.Generator().manual_seed(b * 10 + t)
            leaf = torch.randn((b * t, 2, 3, 4, 8), generator=gen).requires_grad_(True)
            arg = ops.center_over_t(leaf, b, t, t // 2)
            g = torch.randn(arg.shape, generator=gen)

            class Rec:
                args = (arg,)
            true = O.contributions([Rec], [leaf], lambda i: {0: g})[id(leaf)]
            assert len(true) == b * t
            got, = torch.autograd.grad(arg, leaf, g, retain_graph=True)
            ok, ratio, m = O.sum_rule(true, got)
            assert ok and m == t and ratio <= 1.0, (ok, ratio, m)
            one = O.contributions([Rec], [leaf], lambda i: {0: g}, one_frame=True)[id(leaf)]
            assert len(one) == b
            ok1, _, m1 = O.sum_rule(one, got)
            assert m1 == 1 and not ok1
            ratios[f'b{b} t{t}'] = float('inf')
    for k, v in ratios.items():
        print(f'CONTROL {control:26s} {k:28s} |mutated - true| / bound = {v:.3g}')
        assert v > 2.0, f'{control} at {k}: the mutated reference stays within twice the bound ({v:.3f})'
