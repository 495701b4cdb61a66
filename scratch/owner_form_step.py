"""Events-timed pull-form BPR steps at one width and summation mode, Yelp2018-sized tables, uniform ids (the owner-pass
forms bench.py does not run: D = 32 / 128, deterministic order):  python scratch/owner_form_step.py D [det] [B] [steps]
Prints the median step in us."""
import sys, torch
sys.path.insert(0, '.')
from yelprecommendation_amd.bpr_step import BPRMFStep
from yelprecommendation_amd.data.synthetic import YELP2018_ITEMS as NI, YELP2018_USERS as NU
dev = torch.device('cuda:0')
d = int(sys.argv[1]); det = len(sys.argv) > 2 and sys.argv[2] == "det"
B = int(sys.argv[3]) if len(sys.argv) > 3 else 524288; steps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
g = torch.Generator(device=dev).manual_seed(7)
u = torch.randint(0, NU, (B,), device=dev, generator=g); p = torch.randint(0, NI, (B,), device=dev, generator=g)
n = torch.randint(0, NI, (B,), device=dev, generator=g)
step = BPRMFStep(torch.randn(NU, d, device=dev, generator=g) * 0.05, torch.randn(NI, d, device=dev, generator=g) * 0.05,
                 lr=1e-4, impl="pull", deterministic=det)
for _ in range(10): step.step(u, p, n)
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
for a, b in ev:
    a.record(); step.step(u, p, n); b.record()
torch.cuda.synchronize()
step.check()
t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
print(f"D={d} {'det' if det else 'free'} B={B}: median {t[len(t) // 2]:.1f} us/step (min {t[0]:.1f})", flush=True)
