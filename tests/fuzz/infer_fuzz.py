"""Randomised check of the RRDBNet INFERENCE forward (csrc/rrdbnet.hip: forward_body / forward_impl under torch.no_grad(); net_fuzz.py
calls the network with gradients on and so only ever runs the training forward): random (num_feat, num_grow_ch, num_block, scale,
channels, shape), a random Winograd switch (sr_dev_set_wino_f32 0..4) and a random image-group count with sr_dev_set_group_min_wgs(1),
so that small maps split.  The fp32 output is within 1e-4 of the float64 oracle (oracle/rrdbnet_ref.py on .double() tensors) and
bit-identical to the same call with one group.  Exit code 1 on any mismatch."""
import sys, os, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ctypes as C
import torch
import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.utils import synth
from oracle import rrdbnet_ref as R

random.seed(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16
dev = torch.device('cuda:0')
lib = _lib.load()
lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
lib.sr_dev_set_wino_f32.restype = C.c_int
lib.sr_dev_set_group_min_wgs.argtypes = [C.c_int]
lib.sr_dev_set_group_min_wgs.restype = None
bad = 0
worst = 0.0

try:
    for it in range(N):
        scale = random.choice([4, 4, 2, 1])
        cfg = dict(num_in_ch=random.choice([1, 3, 4]), num_out_ch=random.choice([1, 3, 5]), scale=scale,
                   num_feat=random.choice([16, 32, 48, 64, 96]), num_block=random.choice([0, 1, 2]), num_grow_ch=random.choice([16, 32, 64]))
        m = {4: 1, 2: 2, 1: 4}[scale]
        n, h, w = random.choice([1, 2, 3]), m * random.choice([3, 5, 8, 9, 16, 33]), m * random.choice([4, 7, 8, 17, 24, 65])
        mode, groups = random.choice([0, 1, 2, 3, 4]), random.choice([1, 2, 4])
        sd_np = synth.rrdbnet_state_dict(it, **cfg)
        x_np = synth.uniform_input(100 + it, (n, cfg['num_in_ch'], h, w))
        with torch.no_grad():
            y64 = R.rrdbnet_forward(torch.from_numpy(x_np).double(), {k: torch.from_numpy(v).double() for k, v in sd_np.items()}, scale,
                                    cfg['num_block'])
        net = ira.build_network(dict(type='RRDBNet', **cfg)).to(dev).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
        x = torch.from_numpy(x_np).to(dev)
        lib.sr_dev_set_wino_f32(mode)
        lib.sr_dev_set_group_min_wgs(1)
        # RRDBNet._launch takes its output from torch.empty, and the caching allocator would hand the block of a freed one-group
        # output, still holding the right values, to the grouped call: both outputs stay alive, and the grouped call's block is
        # seeded with NaN first (freed, so that the call gets it or another block that never held y1)
        with torch.no_grad():
            _lib.check(lib.sr_set_forward_groups(1), 'sr_set_forward_groups')
            y1 = net(x)
            seed = torch.full_like(y1, float('nan'))
            del seed
            _lib.check(lib.sr_set_forward_groups(groups), 'sr_set_forward_groups')
            yg = net(x)
            y1, yg = y1.cpu(), yg.cpu()
        ey = float((yg.double() - y64).abs().max())
        same = torch.equal(yg, y1)
        ok = ey < 1e-4 and same
        bad += not ok
        worst = max(worst, ey)
        print(f'{it:2d} {cfg} x={n}x{h}x{w} wino {mode} groups {groups}:  out {ey:.1e} {"same bits as one group" if same else "DIFFERS from one group"} '
              f'{"ok" if ok else "MISMATCH"}', flush=True)
finally:
    lib.sr_dev_set_wino_f32(1)
    lib.sr_dev_set_group_min_wgs(0)
    lib.sr_set_forward_groups(0)
print(f'worst error: {worst:.3e}')
print('mismatches:', bad)
sys.exit(1 if bad else 0)
