"""Timeline of the first bucket of every owner workgroup, and the walk iterations of its four waves (library built
with -DYR_STAMPS): python scratch/stamps.py B   (uniform batch)  |  python scratch/stamps.py bench [B]   (step 0 of
bench.py's batch pool, see scripts/owner_walk_balance.py)"""
import sys, ctypes as C, numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'scripts')
from yelprecommendation_amd.bpr_step import BPRMFStep
from yelprecommendation_amd import _lib
dev = torch.device('cuda:0'); nu, ni, d = 31668, 38048, 64
if sys.argv[1] == "bench":
    import owner_walk_balance
    (u, p, n), _, _ = owner_walk_balance.bench_batch(int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 19)
    u, p, n = (torch.from_numpy(a).to(dev) for a in (u, p, n)); B = u.numel()
else:
    B = int(sys.argv[1])
    u = torch.randint(0, nu, (B,), device=dev); p = torch.randint(0, ni, (B,), device=dev); n = torch.randint(0, ni, (B,), device=dev)
step = BPRMFStep(torch.randn(nu, d, device=dev) * 0.05, torch.randn(ni, d, device=dev) * 0.05, lr=1e-4, impl="pull")
for _ in range(20): step.step(u, p, n)
torch.cuda.synchronize()
lib = _lib.load()
buf = np.zeros(8192 * 8, np.int64)
lib.yr_debug_read_stamps.argtypes = [C.c_void_p, C.c_int]
assert lib.yr_debug_read_stamps(buf.ctypes.data, buf.size) == 0
iters = np.zeros(8192 * 4, np.int32)
lib.yr_debug_read_walk_iters.argtypes = [C.c_void_p, C.c_int]
assert lib.yr_debug_read_walk_iters(iters.ctypes.data, iters.size) == 0
per_bucket = torch.bincount(torch.cat([p, n]) >> 4, minlength=(ni + 15) >> 4).cpu().numpy()
for name, lo, nb in (("user", 0, 4096), ("item", 4096, 4096)):
    full = buf.reshape(8192, 8)[lo:lo + nb]
    own = (full[:, :6] > 0).all(1)  # owner workgroups only: helper / sizing workgroups leave no stamps
    s = full[own, :6].astype(np.float64)
    it = iters.reshape(8192, 4)[lo:lo + nb][own].astype(np.float64)
    bucket, heavy_walks = full[own, 6], full[own, 7]
    t0 = s[:, 0].min()
    s = (s - t0) / 100.0           # wall_clock64: 100 MHz -> us
    print(name, "pass:", len(s), "owner workgroups; first start -> last end", round(s[:, 5].max(), 2), "us; last start at", round(s[:, 0].max(), 2), "us")
    for q in (0, len(s) // 4, len(s) // 2, len(s) - 1):
        print("  wg", q, " ".join(f"{x:7.2f}" for x in s[q]))
    dd = np.diff(s, axis=1)
    print("  mean phase us (start->zeroed, ->desc, ->walked, ->stored, ->barrier):", np.round(dd.mean(0), 2),
          " per workgroup", round(float((s[:, 5] - s[:, 0]).mean()), 2), "max", round(float((s[:, 5] - s[:, 0]).max()), 2))
    busy = it.mean(1) > 0
    print(f"  walk iterations of the first bucket: slowest wave mean {it.max(1).mean():.2f}  mean wave {it.mean(1).mean():.2f}  "
          f"slowest / mean (buckets with records) {np.mean(it[busy].max(1) / it[busy].mean(1)):.3f}  heavy-row walks per bucket {heavy_walks.mean():.2f}")
    end = s[:, 4]
    print("  end of the first bucket, us (p10 p50 p90 p99 max):", " ".join(f"{np.percentile(end, q):.1f}" for q in (10, 50, 90, 99, 100)))
    c = np.corrcoef(it.max(1), dd[:, 2])[0, 1]
    print(f"  walk phase us against slowest-wave iterations: correlation {c:.3f}, us per iteration {np.polyfit(it.max(1), dd[:, 2], 1)[0]:.3f}")
    if name == "item":
        k = int(np.argmax(per_bucket[bucket]))
        print(f"  heaviest first bucket: {bucket[k]} with {per_bucket[bucket[k]]} records ends at {end[k]:.1f} us; the pass ends at {s[:, 5].max():.1f} us")
