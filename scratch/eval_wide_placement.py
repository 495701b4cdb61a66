"""The wide f32 sweep (D = 1,024, k = 10, Yelp2018 size, no hints) on the SAME tables at different places in memory, in one
process: fresh allocations (the earlier ones kept alive) and 16-byte-aligned shifted views.  The time has two states
(about 34 and 39.5 ms) that depend on the placement alone: profiles/eval_sweep_pieces_ab.txt.
python scratch/eval_wide_placement.py   (YR_ENGINE_LIB selects another build of the library)"""
import sys, time, json, torch
sys.path.insert(0, '.')
from yelprecommendation_amd import engine
dev = torch.device('cuda:0')
NU, NI, D = 31668, 38048, 1024
g = torch.Generator(device=dev).manual_seed(2)
users = torch.arange(NU, device=dev)
ptr = torch.arange(NU + 1, device=dev, dtype=torch.int64) * 40
idx = engine.sort_mask_rows(ptr, torch.randint(0, NI, (NU * 40,), generator=g, device=dev))
U0 = (torch.rand(NU, D, generator=g, device=dev) - 0.5) * 0.1
I0 = (torch.rand(NI, D, generator=g, device=dev) - 0.5) * 0.1
def tk(U, I, n=5):
    f = lambda: engine.mf_eval_topk(U, I, users, ptr, idx, 10, precision="f32")
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(n):
        t = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return round(sorted(ts)[n // 2] * 1e3, 2)
keep, fresh, shifted = [], [], []
fresh.append(tk(U0, I0))
for trial in range(5):
    pad = torch.empty((trial + 1) * 3 * 1024 * 1024 + 4096 * trial, dtype=torch.uint8, device=dev)
    U, I = U0.clone(), I0.clone()
    keep += [pad, U, I]
    fresh.append(tk(U, I))
for off in (64, 256, 512, 768, 1024 + 64):          # floats: 16-byte aligned shifts of both tables inside one allocation
    Ub = torch.empty(NU * D + 4096, device=dev); Ib = torch.empty(NI * D + 4096, device=dev)
    U = Ub[off:off + NU * D].view(NU, D); U.copy_(U0)
    I = Ib[2 * off:2 * off + NI * D].view(NI, D); I.copy_(I0)
    shifted.append(tk(U, I))
print("RESULT " + json.dumps({"fresh_allocations": fresh, "shifted_views": shifted}))
