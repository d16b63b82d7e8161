"""archs/hip_generator.py on the host (no GPU: the weight images and the weight-gradient launches are stubs): the per-network
weight-image cache of HipGenerator.packed and the cache of derived tensors under it (HipGenerator.derived), the shared forward's
refusals, the parameter order the FlatAdam arena relies on, and GradRouter's routing of parameter gradients."""
from types import SimpleNamespace

import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib, hip_ops
from image_restoration_amd.archs.arch_util import bn_prologue
from image_restoration_amd.archs.hip_generator import GradRouter, HipGenerator

NETS = {
    'MSRResNet': dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, upscale=4),
    'EDSR': dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, upscale=4),
    'RCAN': dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_group=1, num_block=1, squeeze_factor=4, upscale=2),
    'RIDNet': dict(in_channels=3, mid_channels=16, out_channels=3, num_block=1),
}


def _net(kind):
    net = ira.build_network(dict(type=kind, **NETS[kind]))
    assert isinstance(net, HipGenerator)
    return net


def _first_conv(net):
    return net.head if type(net).__name__ == 'RIDNet' else net.conv_first


@pytest.fixture
def built(monkeypatch):
    """Replaces the three weight-image classes by a stub that records (class name, weight, bias, mode)."""
    log = []

    def stub(name):
        def make(w, b=None, mode=0):
            log.append(SimpleNamespace(cls=name, weight=w, bias=b, mode=mode))
            return log[-1]
        return make
    for name in ('PackedConv', 'PackedConvBF16', 'PackedConvK'):
        monkeypatch.setattr(hip_ops, name, stub(name))
    return log


@pytest.mark.parametrize('kind', list(NETS))
def test_packed_hits_and_separate_entries(built, kind):
    net = _net(kind)
    conv = _first_conv(net)
    first = net.packed(conv)
    assert net.packed(conv) is first and net.packed(conv, 0, False) is first and len(built) == 1
    assert (first.cls, first.mode) == ('PackedConv', 0) and first.weight is conv.weight and first.bias is conv.bias
    dgrad = net.packed(conv, 1)
    assert dgrad is not first and dgrad.mode == 1 and dgrad.bias is None and len(built) == 2     # the bias only in mode 0
    half = net.packed(conv, bf16=True)
    assert half.cls == 'PackedConvBF16' and half.bias is conv.bias and len(built) == 3
    assert net.packed(conv, 1) is dgrad and net.packed(conv, 0, True) is half and net.packed(conv) is first and len(built) == 3
    assert set(net._packs) == {(id(conv), 0, False), (id(conv), 1, False), (id(conv), 0, True)}


@pytest.mark.parametrize('kind', list(NETS))
def test_packed_rebuilds_when_the_parameter_changed_behind_it(built, kind):
    net = _net(kind)
    conv = _first_conv(net)
    net.packed(conv)

    def rebuilt_once(what):
        n = len(built)
        pc = net.packed(conv)
        assert len(built) == n + 1 and built[-1] is pc, what
        assert net.packed(conv) is pc and len(built) == n + 1, what

    with torch.no_grad():
        conv.weight.add_(1)                      # torch's version counter
    rebuilt_once('weight.add_')
    with torch.no_grad():
        conv.bias.add_(1)                        # ... the bias's too
    rebuilt_once('bias.add_')
    cell = [0]
    conv.weight._sr_epoch = cell                 # an optimiser that writes through raw pointers (optim.FlatAdam)
    n = len(built)
    net.packed(conv)
    assert len(built) == n                       # epoch 0 is what a parameter without a cell counts as
    cell[0] += 1
    rebuilt_once('_sr_epoch bump')
    net.invalidate_packed()
    rebuilt_once('invalidate_packed')
    if kind == 'RCAN':
        net._affine['cpu'] = object()
    net.double().float()                         # through _apply: new parameter storage, every image dropped
    assert net._packs == {}
    if kind == 'RCAN':
        assert net._affine == {}
    rebuilt_once('_apply')


def test_ridnet_packs_by_kernel_size(built):
    net = _net('RIDNet')
    eam = net.body[0]
    assert net.packed(eam.block2.body[4]).cls == 'PackedConvK' and eam.block2.body[4].weight.shape[2] == 1
    assert net.packed(eam.block2.body[4], 1).cls == 'PackedConvK'
    for conv in (net.head, eam.merge.dilation1[2], eam.merge.aggregation[0], eam.block1.conv1, eam.block2.body[0], net.tail):
        assert net.packed(conv).cls == 'PackedConv' and conv.weight.shape[2] == 3


@pytest.mark.parametrize('kind', list(NETS))
def test_packed_refuses_other_dtypes_by_the_class_name(built, kind):
    net = _net(kind).half()
    with pytest.raises(_lib.SrHipError, match=f'{kind} parameters must be fp32'):
        net.packed(_first_conv(net))
    assert not built


def _derived_setup():
    """A bare HipGenerator that owns three CPU tensors, and a ``get()`` that asks for what is derived from them; ``calls``
    counts the builds."""
    net = HipGenerator()
    net.a = torch.nn.Parameter(torch.ones(3))
    net.register_buffer('b', torch.zeros(2))
    net.register_buffer('c', torch.full((1,), 2.0))
    calls = []

    def build():
        calls.append(1)
        return SimpleNamespace(total=float(net.a.detach().sum() + net.b.sum() + net.c.sum()))

    return net, calls, lambda extra=1e-5: net.derived('sum', (net.a, net.b, net.c), extra, build)


def test_derived_hits_on_an_unchanged_signature():
    net, calls, get = _derived_setup()
    first = get()
    assert first.total == 5.0 and get() is first and get() is first and len(calls) == 1
    assert set(net._packs) == {'sum'}
    assert get(1e-3) is not first and len(calls) == 2          # ``extra`` is part of the signature
    other = net.derived('other', (net.a,), None, lambda: object())
    assert net.derived('other', (net.a,), None, lambda: object()) is other and set(net._packs) == {'sum', 'other'}


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_derived_rebuilds_after_an_in_place_edit_of_any_tensor(name):
    net, calls, get = _derived_setup()
    first = get()
    with torch.no_grad():
        getattr(net, name).add_(1)
    second = get()
    assert second is not first and second.total == first.total + getattr(net, name).numel() and len(calls) == 2
    assert get() is second and len(calls) == 2
    t = getattr(net, name)
    t.data = t.data.clone()                                    # new storage, same values
    assert get() is not second and len(calls) == 3


def test_derived_rebuilds_after_invalidate_packed():
    net, calls, get = _derived_setup()
    first = get()
    net.invalidate_packed()
    second = get()
    assert second is not first and len(calls) == 2 and get() is second and len(calls) == 2


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_derived_rebuilds_after_a_write_behind_the_version_counter(name):
    """FlatAdam writes through raw pointers and bumps the tensor's ``_sr_epoch`` cell: storage and ``_version`` stay."""
    net, calls, get = _derived_setup()
    t = getattr(net, name)
    cell = [0]
    t._sr_epoch = cell
    first = get()
    assert get() is first and len(calls) == 1                  # epoch 0 is what a tensor without a cell counts as
    before = (t.data_ptr(), t._version)
    t.data.add_(1)                                             # .data: no version bump
    cell[0] += 1
    assert (t.data_ptr(), t._version) == before
    second = get()
    assert second is not first and second.total == first.total + t.numel() and len(calls) == 2
    assert get() is second and len(calls) == 2


def test_derived_is_empty_after_apply():
    net, calls, get = _derived_setup()
    get()
    net.derived('other', (net.a,), None, lambda: object())
    net.double().float()
    assert net._packs == {}
    get()
    assert len(calls) == 2 and set(net._packs) == {'sum'}
    with pytest.raises(_lib.SrHipError, match='HipGenerator parameters must be fp32'):
        net.double().derived('sum', (net.a,), None, lambda: calls.append(1))
    assert len(calls) == 2 and net._packs == {}


def test_the_networks_derived_tensors_see_a_write_behind_the_version_counter():
    """The BatchNorm prologue of DUF and the host (mean, std) of SpyNet and TOFlow are written on ``derived``."""
    duf = ira.build_network(dict(type='DUF', scale=2, num_layer=16)).eval()
    bn = duf.bn3d2
    scale, shift = duf.prologue(bn)
    assert duf.prologue(bn)[0] is scale and torch.equal(scale, bn_prologue(bn)[0])
    cell = [0]
    bn.running_var._sr_epoch = cell
    assert duf.prologue(bn)[0] is scale
    bn.running_var.data.mul_(4)
    cell[0] += 1
    assert torch.equal(duf.prologue(bn)[0], bn_prologue(bn)[0]) and not torch.equal(duf.prologue(bn)[0], scale)
    for kind in ('SpyNet', 'TOFlow'):
        net = ira.build_network(dict(type=kind)).eval()
        assert type(net)._norm_host is HipGenerator._norm_host and not hasattr(net, '_norm')
        mean, std = net._norm_host()
        assert net._norm_host()[0] is mean and mean == net.mean.flatten().tolist() and std == net.std.flatten().tolist()
        with torch.no_grad():
            net.std.mul_(2)
        assert net._norm_host()[1] == [2 * s for s in std] and net._norm_host()[0] is not mean


def test_parameter_order_of_the_conv_only_networks():
    """MSRResNet and EDSR use the base's _param_list (registration order); the arena offsets of optim.FlatAdam and the
    positions GradRouter returns gradients at follow it.  It is weight, bias per conv in the order of the layer list."""
    for kind, s in (('MSRResNet', 2), ('MSRResNet', 4), ('EDSR', 3), ('EDSR', 4)):
        net = ira.build_network(dict(type=kind, **dict(NETS[kind], num_block=2, upscale=s)))
        convs = [net.conv_first] + [c for blk in net.body for c in (blk.conv1, blk.conv2)]
        if kind == 'EDSR':
            convs.append(net.conv_after_body)
        convs += [c for c, _ in net.ups()]
        convs += [net.conv_hr, net.conv_last] if kind == 'MSRResNet' else [net.conv_last]
        want = [id(t) for c in convs for t in (c.weight, c.bias)]
        assert [id(p) for p in net._param_list()] == [id(p) for p in net.parameters()] == want, (kind, s)
        assert [k for k, _ in net.named_parameters()] == list(net.state_dict())


@pytest.mark.parametrize('kind', list(NETS))
def test_forward_refuses_a_cpu_input(kind):
    net = _net(kind)
    for x in (torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8, requires_grad=True)):
        with pytest.raises(_lib.SrHipError, match=f'{kind}.forward runs only on a HIP device'):
            net(x)


# ----------------------------------------------------------------------------------------------------------------- GradRouter
def _router_net():
    net = _net('RIDNet')
    params = net._param_list()
    return net, params, SimpleNamespace(grad_ptrs=[1000 + 8 * i for i in range(len(params))])


def test_router_arena_is_all_or_nothing():
    net, params, sink = _router_net()
    net._grad_sink = sink
    need = [True] * len(params)
    assert GradRouter(net, params, need).to_sink
    need[3] = False
    with pytest.raises(_lib.SrHipError, match='flat-arena mode needs every generator parameter to require grad'):
        GradRouter(net, params, need)
    assert not GradRouter(net, params, [False] * len(params)).to_sink      # nothing to route: the arena is left alone


def test_router_targets_with_and_without_an_arena():
    net, params, sink = _router_net()
    ca = net.body[0].ca
    ps = (ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias)
    frozen = {id(ca.fc1.bias), id(ca.fc2.weight)}
    router = GradRouter(net, params, [id(p) not in frozen for p in params])
    ptrs, acc = router.targets(ps)
    assert acc is False
    for p, ptr in zip(ps, ptrs):
        i = router.index[id(p)]
        assert params[i] is p
        if id(p) in frozen:
            assert ptr is None and router.grads[i] is None
        else:
            g = router.grads[i]
            assert g.shape == p.shape and g.dtype == p.dtype and ptr == g.data_ptr()
    assert sum(g is not None for g in router.grads) == 2
    net._grad_sink = sink
    router = GradRouter(net, params, [True] * len(params))
    ptrs, acc = router.targets(ps)
    assert acc is True and ptrs == tuple(sink.grad_ptrs[router.index[id(p)]] for p in ps)
    assert all(g is None for g in router.grads)


def test_router_wgrad_launches_only_what_is_wanted(monkeypatch):
    net, params, sink = _router_net()
    calls = []

    def dense(src, d, cout, cin, *, scale=1.0, out=None):
        calls.append(('conv3x3_wgrad', cout, cin, scale, out))
        return ('dw', 'db') if out is None else None

    def other(src, d, cout, cin, ksize=3, dilation=1, *, scale=1.0, out=None):
        calls.append(('convd_wgrad', cout, cin, ksize, dilation, scale, out))
        return ('dw', 'db') if out is None else (None, None)
    monkeypatch.setattr(hip_ops, 'conv3x3_wgrad', dense)
    monkeypatch.setattr(hip_ops, 'convd_wgrad', other)
    head, one = net.head, net.body[0].block2.body[4]
    frozen = {id(head.weight), id(head.bias), id(net.tail.bias)}
    router = GradRouter(net, params, [id(p) not in frozen for p in params])
    router.wgrad(head, None, None)
    assert calls == [] and router.grads[router.index[id(head.weight)]] is None       # both frozen: no launch at all
    router.wgrad(net.tail, None, None, scale=0.5)
    assert calls == [('conv3x3_wgrad', 3, 16, 0.5, None)]
    assert router.grads[router.index[id(net.tail.weight)]] == 'dw' and router.grads[router.index[id(net.tail.bias)]] is None
    router.wgrad(one, None, None)                                                   # 1x1: the general kernel
    router.wgrad(net.body[0].merge.dilation1[2], None, None, dilation=2)            # 3x3 dilated: the general kernel too
    assert calls[1:] == [('convd_wgrad', 16, 16, 1, 1, 1.0, None), ('convd_wgrad', 16, 16, 3, 2, 1.0, None)]
    assert router.grads[router.index[id(one.bias)]] == 'db'
    # arena: every launch adds in place through the sink's pointers, nothing is returned to autograd
    del calls[:]
    net._grad_sink = sink
    router = GradRouter(net, params, [True] * len(params))
    router.wgrad(head, None, None)
    iw, ib = router.index[id(head.weight)], router.index[id(head.bias)]
    assert calls == [('conv3x3_wgrad', 16, 3, 1.0, (sink.grad_ptrs[iw], sink.grad_ptrs[ib]))]
    assert all(g is None for g in router.grads)


# ------------------------------------------------------------------------------------------------------- arch_util.upscale_stages
def test_upscale_edges_keep_each_networks_own_rule():
    """One stage list, two acceptance rules: EDSR follows the reference's Upsample (any 2^n int from 1, or anything equal to 3),
    RCAN takes ints from 2 only; each refuses in its own words."""
    from image_restoration_amd.archs.arch_util import upscale_stages
    assert [upscale_stages(s) for s in (1, 2, 3, 4, 8, 3.0)] == [[], [2], [3], [2, 2], [2, 2, 2], [3]]
    assert [upscale_stages(s) for s in (0, -2, 5, 6, 2.0, 4.0, '3', None)] == [None] * 8
    edsr = dict(type='EDSR', num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1)
    assert [c.out_channels for c, _ in ira.build_network(dict(edsr, upscale=3.0)).ups()] == [144]
    assert ira.build_network(dict(edsr, upscale=1)).ups() == [] and ira.build_network(dict(edsr, upscale=True)).ups() == []
    for s in (2.0, 5, 0):
        with pytest.raises(ValueError, match='Supported scales: 2\\^n and 3'):
            ira.build_network(dict(edsr, upscale=s))
    for s in (3.0, 2.0, True, False, 1, 0, 6):
        with pytest.raises(ValueError, match='RCAN supports upscale 2\\^n \\(n >= 1\\) and 3'):
            ira.build_network(dict(type='RCAN', **dict(NETS['RCAN'], upscale=s)))
