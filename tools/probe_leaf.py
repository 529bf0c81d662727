import sys, numpy as np, torch
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygpr_amd._ops import get_ops
ops = get_ops()
rng = np.random.default_rng(0)
nb = 64
mats = []
for _ in range(nb):
    a = rng.standard_normal((128, 128)); mats.append(a @ a.T / 128 + np.eye(128))
src = torch.from_numpy(np.stack(mats)).cuda()
inv = torch.zeros(nb, 128, 128, device="cuda", dtype=torch.float64)
info = torch.zeros(1, dtype=torch.int32, device="cuda")
def run():
    a = src.clone(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for b in range(nb): ops.leaf_raw(a[b], inv[b], info)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / nb * 1e3
run(); t = min(run() for _ in range(3))
print(f"{'full':50s} {t:7.1f} us per leaf", flush=True)
