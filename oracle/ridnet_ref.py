"""Oracle: plain PyTorch-CPU functional restatement of the reference's RIDNet (basicsr/archs/ridnet_arch.py), run in float64
by the tests.

TEST INFRASTRUCTURE — not shipped, not measured as the product.  Pinned against the reference itself: tools/make_golden_ridnet.py
runs the reference's own modules on seeded weights and inputs and commits the outputs and float64 gradients to
tests/golden/g_w_ridnet.npz; tests/test_oracle.py checks this file (forward and autograd backward) against those vectors.  Every
function cites the reference lines it follows.

Parameters are passed as a flat dict name -> tensor with the reference's state_dict keys; the computation runs in the dtype of
the input and the parameters (pass float64 for a float64 oracle).
"""
import torch
import torch.nn.functional as F


def _t(v):
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(v)


def conv(x, sd, name, padding=0, dilation=1):
    """nn.Conv2d(cin, cout, k, 1, padding, dilation) with its bias."""
    return F.conv2d(x, _t(sd[f'{name}.weight']), _t(sd[f'{name}.bias']), padding=padding, dilation=dilation)


def merge_run(x, sd, prefix):
    """MergeRun (ridnet_arch.py:72-88): two branches of dilations 1, 2 and 3, 4, each conv followed by a ReLU, their concat
    through a 3x3 conv and a ReLU, plus the input."""
    d1 = F.relu(conv(x, sd, f'{prefix}dilation1.0', 1, 1))
    d1 = F.relu(conv(d1, sd, f'{prefix}dilation1.2', 2, 2))
    d2 = F.relu(conv(x, sd, f'{prefix}dilation2.0', 3, 3))
    d2 = F.relu(conv(d2, sd, f'{prefix}dilation2.2', 4, 4))
    out = F.relu(conv(torch.cat([d1, d2], 1), sd, f'{prefix}aggregation.0', 1))
    return out + x


def residual_block(x, sd, prefix):
    """ResidualBlockNoBN (arch_util.py:84-87, res_scale 1): x + conv2(relu(conv1(x)))."""
    return x + conv(F.relu(conv(x, sd, f'{prefix}conv1', 1)), sd, f'{prefix}conv2', 1)


def eresidual_block(x, sd, prefix):
    """EResidualBlockNoBN (ridnet_arch.py:44-56): conv3x3-ReLU-conv3x3-ReLU-conv1x1, plus the input, then a ReLU."""
    out = F.relu(conv(x, sd, f'{prefix}body.0', 1))
    out = F.relu(conv(out, sd, f'{prefix}body.2', 1))
    out = conv(out, sd, f'{prefix}body.4', 0)
    return F.relu(out + x)


def channel_attention(x, sd, prefix):
    """ChannelAttention (ridnet_arch.py:101-107): x * sigmoid(conv(relu(conv(mean_hw x)))), no identity."""
    y = x.mean((2, 3), keepdim=True)
    y = F.relu(conv(y, sd, f'{prefix}attention.1'))
    y = torch.sigmoid(conv(y, sd, f'{prefix}attention.3'))
    return x * y


def eam(x, sd, prefix):
    """EAM.forward (ridnet_arch.py:133-138)."""
    out = merge_run(x, sd, f'{prefix}merge.')
    out = F.relu(residual_block(out, sd, f'{prefix}block1.'))
    out = eresidual_block(out, sd, f'{prefix}block2.')
    return channel_attention(out, sd, f'{prefix}ca.')


def ridnet_forward(x, sd, num_block=4):
    """RIDNet.forward (ridnet_arch.py:178-184): MeanShift layers are 3 -> 3 1x1 convs (ridnet_arch.py:21-28)."""
    x = _t(x)
    res = conv(x, sd, 'sub_mean')
    res = F.relu(conv(res, sd, 'head', 1))
    for b in range(num_block):
        res = eam(res, sd, f'body.{b}.')
    res = conv(res, sd, 'tail', 1)
    res = conv(res, sd, 'add_mean')
    return x + res
