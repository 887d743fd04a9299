"""tests/golden/wino2d_d1.npz: forward, data gradient and weight gradient of the undilated 2-D Winograd F(2x2, 3x3) layer
(1 x 64 -> 64 x 8 x 12, seeded inputs) as computed on the GPU by the tree this script is run from.  The committed file was
written on the commit before ssbev_wino_dims got its dilation, so that tests/test_gpu_wino2d_dilated.py can hold d = 1 to that
commit's bits.  usage: python tools/make_golden_wino2d_d1.py [out.npz]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from stereoscene_amd import functional as F, synthetic as S

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                         "wino2d_d1.npz")
x = S.hash_normal("wino2d_d1/x", (1, 64, 8, 12)).cuda().requires_grad_(True)
w = (S.hash_uniform("wino2d_d1/w", (64, 64, 3, 3), -1, 1) * (3.0 / (64 * 9)) ** 0.5).cuda().requires_grad_(True)
go = S.hash_normal("wino2d_d1/go", (1, 64, 8, 12)).cuda()
assert F._WinoConv._plan(False, 1, 8, 12, False)[1] == "ssbev_wino2d_"
y = F.conv2d(x, w, None, 1, 1, 1)
y.backward(go)
torch.cuda.synchronize()
np.savez(out, y=y.detach().cpu().numpy(), gx=x.grad.cpu().numpy(), gw=w.grad.cpu().numpy())
print(out, os.path.getsize(out), "bytes")
