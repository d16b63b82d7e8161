"""archs/hip_driver.py on the host (no GPU): what RRDBNet, the VGG-style discriminators and the U-Net discriminator inherit for
their whole-network entry points.  The loaded library is the recorder of tests/test_binding_host.py (size queries go through,
pack calls are recorded), parameters are CPU tensors: when a weight blob is rebuilt, what the cached parameter walk is dropped by,
where a backward's parameter gradients go, and the two workspace policies."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch
from torch import nn

import image_restoration_amd as ira
from image_restoration_amd import _lib, hip_ops
from image_restoration_amd.archs import hip_driver
from image_restoration_amd.archs.hip_driver import device_input, grad_targets, grow_workspace, symbol

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_binding_host import _calls, rec  # noqa: E402, F401

NETS = {'RRDBNet': dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8),
        'VGGStyleDiscriminator128': dict(num_in_ch=3, num_feat=16)}
STREAM = 0x77


def _net(kind, **kw):
    net = ira.build_network(dict(type=kind, **dict(NETS[kind], **kw)))
    assert isinstance(net, hip_driver.HipDriverNet)
    return net


def _kinds(net):
    """The arguments of net._packed for every blob the network keeps."""
    if type(net).__name__ == 'RRDBNet':
        return [dict(bf16=b, dgrad=d) for b in (False, True) for d in (False, True)]
    return [dict(bf16=b) for b in (False, True)]


def _pack_all(net):
    lib, cfg = _lib.load(), net._cfg()
    return [net._packed(lib, cfg, STREAM, **kw) for kw in _kinds(net)]


def _names(rec):  # noqa: F811
    return [name for name, _ in _calls(rec)]


PACKS = {'RRDBNet': ['sr_rrdbnet_pack_f32', 'sr_rrdbnet_pack_dgrad_f32', 'sr_rrdbnet_pack_bf16', 'sr_rrdbnet_pack_dgrad_bf16'],
         'VGGStyleDiscriminator128': ['sr_vgg_pack_f32', 'sr_vgg_pack_bf16']}


# ------------------------------------------------------------------------------------------------------------ invalidation
def _write_in_place(net):
    with torch.no_grad():
        net._param_list()[0].add_(1)          # the first conv weight: every image holds it


def _bump_cell(net):
    net._param_list()[0]._sr_epoch[0] += 1   # what optim.FlatAdam does per fused step


def _reallocate(net, keep=[]):
    p = net._param_list()[0]
    keep.append(p.data)                       # the old storage stays alive: its address cannot come back
    p.data = p.data.clone()


WRITERS = {'in-place write': _write_in_place, 'invalidate_packed': lambda net: net.invalidate_packed(),
           'hip_ops.invalidate_packs': lambda net: hip_ops.invalidate_packs(), '_sr_epoch bump': _bump_cell,
           're-allocated parameter': _reallocate}


@pytest.mark.parametrize('writer', list(WRITERS))
@pytest.mark.parametrize('kind', list(NETS))
def test_every_blob_is_rebuilt_once_per_change_and_never_without(rec, kind, writer):  # noqa: F811
    net = _net(kind)
    net._param_list()[0]._sr_epoch = [0]      # epoch 0 is what a parameter without a cell counts as: set before the first pack
    first = _pack_all(net)
    assert _names(rec) == PACKS[kind]
    params = net._param_list()
    for (name, args), blob in zip(_calls(rec), first):
        assert [args[1][i] for i in range(len(params))] == [p.data_ptr() for p in params]     # state_dict order
        assert args[2] == blob.data_ptr() and args[3] == STREAM and blob.dtype == torch.uint8
    again = _pack_all(net)
    assert all(a is b for a, b in zip(first, again)) and len(_calls(rec)) == len(first)       # untouched: nothing
    WRITERS[writer](net)
    _pack_all(net)
    assert _names(rec) == PACKS[kind] * 2, writer
    _pack_all(net)
    assert len(_calls(rec)) == 2 * len(first), writer


def test_one_nets_invalidation_leaves_another_nets_blobs_alone(rec):  # noqa: F811
    nets = [_net('RRDBNet'), _net('RRDBNet'), _net('VGGStyleDiscriminator128')]
    for net in nets:
        _pack_all(net)
    del rec.log[:]
    nets[0].invalidate_packed()
    _pack_all(nets[1])
    _pack_all(nets[2])
    assert _calls(rec) == []
    _pack_all(nets[0])
    assert _names(rec) == PACKS['RRDBNet']


def test_a_bias_write_repacks_the_forward_images_and_not_the_data_gradient_ones(rec):  # noqa: F811
    net = _net('RRDBNet')
    _pack_all(net)
    del rec.log[:]
    with torch.no_grad():
        net.conv_last.bias.add_(1)
    _pack_all(net)
    assert _names(rec) == ['sr_rrdbnet_pack_f32', 'sr_rrdbnet_pack_bf16']
    with torch.no_grad():
        net.conv_body.weight.add_(1)
    _pack_all(net)
    assert _names(rec)[2:] == PACKS['RRDBNet']


@pytest.mark.parametrize('kind', list(NETS))
def test_a_repack_of_the_same_size_reuses_the_allocation(rec, kind):  # noqa: F811
    net = _net(kind)
    first = _pack_all(net)
    lib, cfg = _lib.load(), net._cfg()
    sizes = {'RRDBNet': [lib.sr_rrdbnet_packed_bytes, lib.sr_rrdbnet_packed_dgrad_bytes, lib.sr_rrdbnet_packed_bytes_bf16,
                         lib.sr_rrdbnet_packed_dgrad_bytes_bf16],
             'VGGStyleDiscriminator128': [lib.sr_vgg_packed_bytes, lib.sr_vgg_packed_bytes_bf16]}[kind]
    assert [b.numel() for b in first] == [q(C.byref(cfg)) for q in sizes]
    net.invalidate_packed()
    again = _pack_all(net)
    assert all(a is b for a, b in zip(first, again)) and len(_calls(rec)) == 2 * len(first)
    assert len({b.data_ptr() for b in first}) == len(first)                                   # one allocation per kind


# ------------------------------------------------------------------------------------- the checks each image has always had
def test_the_parameter_checks_each_pack_keeps(rec):  # noqa: F811
    lib = _lib.load()
    half = _net('RRDBNet').half()
    for bf16 in (False, True):
        with pytest.raises(_lib.SrHipError, match='^RRDBNet parameters must be contiguous fp32 on one HIP device$'):
            half._packed(lib, half._cfg(), STREAM, bf16)
    assert _calls(rec) == []
    half._packed(lib, half._cfg(), STREAM, False, dgrad=True)   # the data-gradient pack never looked at the dtype (it runs after a forward)
    assert _names(rec) == ['sr_rrdbnet_pack_dgrad_f32']
    vgg = _net('VGGStyleDiscriminator128').half()
    with pytest.raises(_lib.SrHipError, match='^discriminator parameters must be contiguous fp32 on one HIP device$'):
        vgg._packed(lib, vgg._cfg(), STREAM, False)
    # the count: the fp32 forward pack and the discriminator's ask sr_*_num_params, RRDBNet's bf16 and data-gradient packs never did
    net = _net('RRDBNet')
    deeper = _net('RRDBNet', num_block=2)
    have, want = len(net._param_list()), len(deeper._param_list())
    with pytest.raises(_lib.SrHipError, match=f'^parameter count {have} != {want} expected by libsr_hip.so$'):
        net._packed(lib, deeper._cfg(), STREAM, False)
    net._packed(lib, deeper._cfg(), STREAM, True)
    vgg = _net('VGGStyleDiscriminator128')
    have, want = len(vgg._param_list()), len(list(ira.build_network(dict(type='VGGStyleDiscriminator256', **NETS[type(vgg).__name__])).parameters()))
    for bf16 in (False, True):
        with pytest.raises(_lib.SrHipError, match=f'^parameter count {have} != {want} expected by libsr_hip.so$'):
            vgg._packed(lib, _lib.VGGCfg(3, 16, 256), STREAM, bf16)
    assert _names(rec) == ['sr_rrdbnet_pack_dgrad_f32', 'sr_rrdbnet_pack_bf16']


@pytest.mark.parametrize('kind, kw, called, named', [
    ('RRDBNet', dict(bf16=False), 'sr_rrdbnet_pack_f32', 'sr_rrdbnet_pack_f32'),
    ('RRDBNet', dict(bf16=True), 'sr_rrdbnet_pack_bf16', 'sr_rrdbnet_pack_bf16'),
    ('RRDBNet', dict(bf16=False, dgrad=True), 'sr_rrdbnet_pack_dgrad_f32', 'sr_rrdbnet_pack_dgrad'),
    ('RRDBNet', dict(bf16=True, dgrad=True), 'sr_rrdbnet_pack_dgrad_bf16', 'sr_rrdbnet_pack_dgrad'),
    ('VGGStyleDiscriminator128', dict(bf16=False), 'sr_vgg_pack_f32', 'sr_vgg_pack'),
    ('VGGStyleDiscriminator128', dict(bf16=True), 'sr_vgg_pack_bf16', 'sr_vgg_pack'),
])
def test_a_failing_pack_keeps_its_error_text_and_is_not_cached(rec, kind, kw, called, named):  # noqa: F811
    net = _net(kind)
    rec.status[called] = 7
    with pytest.raises(_lib.SrHipError) as e:
        net._packed(_lib.load(), net._cfg(), STREAM, **kw)
    assert re.match(re.escape(named) + r' failed \(status 7\): ', str(e.value))
    rec.status.clear()
    net._packed(_lib.load(), net._cfg(), STREAM, **kw)
    assert _names(rec) == [called, called]


def test_symbol_names_both_schemes():
    lib = SimpleNamespace(sr_x_f32=1, sr_x_bf16=2, sr_x=3)
    assert symbol(lib, 'sr_x', False) == (1, 'sr_x_f32') and symbol(lib, 'sr_x', True) == (2, 'sr_x_bf16')
    assert symbol(lib, 'sr_x', False, query=True) == (3, 'sr_x') and symbol(lib, 'sr_x', True, query=True) == (2, 'sr_x_bf16')
    assert symbol(lib, 'sr_x', False, short=True) == (1, 'sr_x') and symbol(lib, 'sr_x', True, short=True) == (2, 'sr_x')


def test_a_cpu_input_is_refused_by_name():
    for kind, x in (('RRDBNet', torch.zeros(1, 3, 8, 8)), ('VGGStyleDiscriminator128', torch.zeros(1, 3, 128, 128))):
        with pytest.raises(_lib.SrHipError, match=re.escape(f'{kind}.forward runs only on a HIP device (no CPU fallback)')):
            _net(kind)(x)
    with pytest.raises(_lib.SrHipError, match=r'^UNetDiscriminatorSN runs only on a HIP device \(no CPU fallback\)$'):
        device_input(torch.zeros(2), 'UNetDiscriminatorSN')


# -------------------------------------------------------------------------------------------------------------- param list
def _middle(net):
    return net.conv_body if type(net).__name__ == 'RRDBNet' else net.conv2_0


@pytest.mark.parametrize('kind', list(NETS))
def test_the_cached_walk_is_dropped_by_apply_and_by_a_new_end(kind):
    net = _net(kind)
    walk = net._param_list()
    assert net._param_list() is walk and [id(p) for p in walk] == [id(p) for p in net.parameters()]
    assert list(net.state_dict())[:1] == [k for k, _ in net.named_parameters()][:1]
    if kind != 'RRDBNet':
        ptrs = net._buffer_ptrs()
        assert net._buffer_ptrs() is ptrs and len(ptrs) == len(list(net.buffers()))
    net.double().float()                          # through _apply
    assert net._plist is None and (kind == 'RRDBNet' or net._bufptrs is None)
    walk = net._param_list()
    assert [id(p) for p in walk] == [id(p) for p in net.parameters()]
    if kind != 'RRDBNet':
        net._buffer_ptrs()
    first_conv = net.conv_first if kind == 'RRDBNet' else net.conv0_0
    first_conv.weight = nn.Parameter(first_conv.weight.detach().clone())      # a new first parameter: the shortcut sees it
    assert net._param_list() is not walk and net._param_list()[0] is first_conv.weight
    assert kind == 'RRDBNet' or net._bufptrs is None


@pytest.mark.parametrize('kind', list(NETS))
def test_debug_packs_catches_a_parameter_re_registered_in_the_middle(monkeypatch, kind):
    monkeypatch.setattr(hip_driver, '_DEBUG_PARAM_LIST', False)
    net = _net(kind)
    walk = net._param_list()
    conv = _middle(net)
    conv.weight = nn.Parameter(conv.weight.detach().clone())
    assert net._param_list() is walk              # the shortcut looks at the two ends only ...
    monkeypatch.setattr(hip_driver, '_DEBUG_PARAM_LIST', True)     # ... SR_DEBUG_PACKS=1 walks the tree every time and says so
    with pytest.raises(AssertionError, match='a parameter in the middle of the network was re-registered'):
        net._param_list()
    net._apply(lambda t: t)
    assert any(p is conv.weight for p in net._param_list())


# -------------------------------------------------------------------------------------------------------- gradient targets
ARENA = 'flat-arena mode needs every generator parameter to require grad'
VGG = 'the whole-network discriminator backward needs all parameters to require grad or none'
UNET = 'the whole-network U-Net backward needs all weights to require grad or none'


def _params():
    ps = [torch.zeros(4, 3, 3, 3), torch.zeros(4), torch.zeros(2, 4, 3, 3), torch.zeros(2)]
    return ps, SimpleNamespace(grad_ptrs=[0x9000 + 64 * i for i in range(len(ps))])


def _fresh(grads, ptrs, items):
    for g, ptr, p in zip(grads, ptrs, items):
        shape = tuple(p.shape) if isinstance(p, torch.Tensor) else p
        assert tuple(g.shape) == shape and g.dtype == torch.float32 and g.is_contiguous() and ptr == g.data_ptr()


def test_gradient_targets_of_the_generator():
    ps, sink = _params()
    yes, no = (True,) * 4, (False,) * 4
    grads, ptrs, acc = grad_targets(ps, yes, sink, ARENA, pairs=True)              # arena: added in place, autograd sees none
    assert grads == [None] * 4 and list(ptrs) == sink.grad_ptrs and acc == 1
    with pytest.raises(_lib.SrHipError, match=f'^{ARENA}$'):
        grad_targets(ps, (True, True, False, False), sink, ARENA, pairs=True)      # ... and all or nothing
    for s in (sink, None):                                                         # nothing wanted: an array of NULLs, as ever
        grads, ptrs, acc = grad_targets(ps, no, s, ARENA, pairs=True)
        assert grads == [None] * 4 and list(ptrs) == [None] * 4 and acc == 0
    grads, ptrs, acc = grad_targets(ps, yes, None, ARENA, pairs=True)
    _fresh(grads, ptrs, ps)
    assert acc == 0
    grads, ptrs, acc = grad_targets(ps, (False, False, True, True), None, ARENA, pairs=True)   # a frozen (weight, bias) pair
    assert grads[:2] == [None, None] and list(ptrs)[:2] == [None, None] and acc == 0
    _fresh(grads[2:], list(ptrs)[2:], ps[2:])
    grads, ptrs, acc = grad_targets(ps, (True, False, True, True), None, ARENA, pairs=True)    # a weight without its bias
    assert grads[1] is None and ptrs[1] is None and grads[0] is not None
    with pytest.raises(_lib.SrHipError, match='^bias.requires_grad without weight.requires_grad is not supported$'):
        grad_targets(ps, (False, True, True, True), None, ARENA, pairs=True)


def test_gradient_targets_of_the_discriminators():
    ps, sink = _params()
    yes, no = (True,) * 4, (False,) * 4
    grads, ptrs, acc = grad_targets(ps, yes, sink, VGG)
    assert grads == [None] * 4 and list(ptrs) == sink.grad_ptrs and acc == 1
    grads, ptrs, acc = grad_targets(ps, yes, None, VGG)
    _fresh(grads, ptrs, ps)
    assert acc == 0
    for s in (sink, None):
        assert grad_targets(ps, no, s, VGG) == ([None] * 4, None, 0)
        with pytest.raises(_lib.SrHipError, match=f'^{VGG}$'):
            grad_targets(ps, (True, True, False, False), s, VGG)
    shapes = [tuple(p.shape) for p in ps]                                          # the U-Net: shapes of temporaries, no arena
    grads, ptrs, acc = grad_targets(shapes, yes, None, UNET, dev=torch.device('cpu'))
    _fresh(grads, ptrs, shapes)
    assert acc == 0
    assert grad_targets(shapes, no, None, UNET, dev=torch.device('cpu')) == ([None] * 4, None, 0)
    with pytest.raises(_lib.SrHipError, match=f'^{UNET}$'):
        grad_targets(shapes, (False, True, True, True), None, UNET, dev=torch.device('cpu'))


# -------------------------------------------------------------------------------------------------------------- workspaces
def test_the_forward_workspace_holds_one_shape_exactly_sized(rec):  # noqa: F811
    net = _net('RRDBNet')
    lib, cfg, dev = _lib.load(), net._cfg(), torch.device('cpu')
    seen = []
    for bf16, shape in ((False, (1, 16, 16)), (False, (1, 16, 16)), (False, (2, 8, 24)), (False, (1, 16, 16)), (True, (1, 16, 16)),
                        (True, (1, 16, 16)), (True, (1, 8, 8))):
        ws, nbytes = net._workspace(lib, cfg, *shape, dev, bf16)
        query = lib.sr_rrdbnet_workspace_bytes_bf16 if bf16 else lib.sr_rrdbnet_workspace_bytes
        assert nbytes == query(C.byref(cfg), *shape) > 0 and ws.numel() == nbytes and ws.dtype == torch.uint8
        assert len(net._workspaces) == 1 and next(iter(net._workspaces.values())) is ws
        seen.append(ws)
    assert seen[1] is seen[0] and seen[2] is not seen[0] and seen[3] is not seen[0] and seen[4] is not seen[3] and seen[5] is seen[4]
    for bf16 in (False, True):                    # an entry smaller than the query says is not handed out (either dtype)
        ws, nbytes = net._workspace(lib, cfg, 1, 16, 16, dev, bf16)
        key, = net._workspaces
        net._workspaces[key] = small = torch.empty(nbytes - 1, dtype=torch.uint8)
        ws, _ = net._workspace(lib, cfg, 1, 16, 16, dev, bf16)
        assert ws is not small and ws.numel() == nbytes and list(net._workspaces) == [key]
    odd = _net('RRDBNet', scale=2)
    with pytest.raises(AssertionError, match='input 15x16 is not divisible by the pixel_unshuffle factor 2'):
        odd._workspace(lib, odd._cfg(), 1, 15, 16, dev, False)
    with pytest.raises(_lib.SrHipError, match='^sr_rrdbnet_workspace_bytes_bf16 returned 0 for input 15x16$'):
        odd._workspace(lib, odd._cfg(), 1, 15, 16, dev, True)


def test_the_grow_only_workspace_never_shrinks_and_follows_the_device():
    for net in (_net('RRDBNet'), ira.build_network(dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=16))):
        assert net._grown == {}
        cpu, meta = torch.device('cpu'), torch.device('meta')
        a = grow_workspace(net, 'bwd', 100, cpu)
        assert a.numel() == 100 and a.dtype == torch.uint8 and grow_workspace(net, 'bwd', 40, cpu) is a
        b = grow_workspace(net, 'bwd', 101, cpu)
        assert b is not a and b.numel() == 101 and grow_workspace(net, 'bwd', 100, cpu) is b
        c = grow_workspace(net, 'bwd', 8, meta)                                   # another device: replaced, however small
        assert c.device == meta and c.numel() == 8 and net._grown['bwd'] is c
        assert grow_workspace(net, 'other', 8, cpu) is not c and set(net._grown) == {'bwd', 'other'}
