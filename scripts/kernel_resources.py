#!/usr/bin/env python3
"""Register / LDS / scratch figures of every kernel in the built objects, read from the gfx950 code objects
(llvm-objdump --offloading + llvm-readelf --notes: the amdhsa.kernels metadata), and the occupancy budgets the
design depends on.  No GPU needed: `__graft_entry__.build()` calls check() after `make`, and so does a CPU test —
an edit that pushes a kernel over its budget fails the build instead of silently halving its occupancy
(the owner passes need 8 workgroups per CU, the split evaluation kernel 3 waves per SIMD).

    python scripts/kernel_resources.py            # table of all kernels + budget check
    python scripts/kernel_resources.py --isa DIR  # ... and the instruction text of every kernel, one file each, so
                                                  # that two builds can be compared with `diff -r` (a refactor that
                                                  # moves code between files must leave them equal)
"""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yelprecommendation_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"

# (regex on the demangled kernel name, max VGPRs (arch + acc), max LDS bytes (static), why)
BUDGETS = [
    (r"void yr::mf_eval_topk_kernel<64, 10, (true|false), true, false>", 168, 54 * 1024,
     "split-form sweep, 10-entry lists: three waves per SIMD (512 / 3 -> 168) and three workgroups per CU"),
    (r"void yr::mf_eval_topk_kernel<64, 4, (true|false), true, false>", 168, 54 * 1024, "as above, 4-entry lists"),
    (r"void yr::mf_eval_topk_kernel<64, 10, (true|false), false, false>", 168, 54 * 1024, "f32-instruction sweep: three workgroups per CU"),
    (r"void yr::owner_pass_kernel<64, (true|false)", 64, 20 * 1024,
     "every bucket's workgroup resident at once: 8 workgroups of 256 threads per CU = 64 VGPRs, <= 20 KB LDS"),
    (r"void yr::owner_pass_kernel<(16|32|128), (true|false)", 64, 20 * 1024, "as above for the other widths"),
    (r"void yr::spmm_csr_kernel<64, (true|false), (true|false)>", 96, 0,
     "one wave per row with 8 gather passes in flight: five waves per SIMD (full and row-subset forms)"),
    (r"void yr::ngcf_dense_fwd_kernel<64, false>", 128, 0, "one wave per workgroup, four waves per SIMD"),
    (r"void yr::ngcf_dense_bwd_data_kernel<64, false>", 128, 0, "as the forward kernel"),
    (r"void yr::ngcf_dense_(fwd|bwd_data)_kernel<64, true>", 168, 0,
     "row-list forms: three waves per SIMD (a hoisted weight tile once took the forward kernel to 252)"),
    # the wide widths (256 / 512 / 1024) of BPR-MF
    (r"void yr::bpr_fwd_bwd_kernel<(256|512|1024), (true|false), (16|64|256)>", 96, 4 * 1024,
     "push form, wide rows: 24 row registers in flight (RowGeom::UNROLL), five waves per SIMD (512 / 5 -> 96)"),
    (r"void yr::mf_score(_backward)?_kernel<(256|512|1024)>", 64, 4 * 1024, "as the narrow widths: eight waves per SIMD"),
    (r"void yr::mf_eval_topk_wide_kernel<(256|512|1024), (4|10|16), (true|false), (true|false)>", 256, 72 * 1024,
     "slab sweep: two workgroups of four waves per CU = two waves per SIMD (512 / 2 -> 256), 2 x 72 KB of 160 KB LDS"),
    (r"void yr::mf_scores_mfma_wide_kernel<(256|512|1024)>", 256, 72 * 1024, "score GEMM in slabs: as the sweep"),
    (r"void yr::et_hint_bound_kernel<(256|512|1024)>", 64, 0, "the dot product is a loop: eight waves per SIMD"),
    # NGCF's evaluation sweep over the layer tables
    (r"void yr::ngcf_eval_topk_kernel<(16|32|64), (4|10|16)>", 168, 40 * 1024,
     "layered sweep: a layer's half row (D / 2 registers) beside two accumulators and the list, at least three "
     "workgroups per CU (512 / 3 -> 168; 36 KB of LDS each: two 32-item tiles of one to four layers + the candidate buffers)"),
    (r"void yr::ngcf_eval_topk_kernel<128, (4|10|16)>", 256, 52 * 1024,
     "as the wide sweep's slab of 128 dims: two workgroups per CU (512 / 2 -> 256), 2 x 49 KB of LDS"),
    (r"void yr::ngcf_hint_bound_kernel<(16|32|64|128)>", 64, 0, "the dot product is a loop over the layers: eight waves per SIMD"),
    (r"void yr::adam_dual_wide_kernel<(true|false)>", 64, 1024, "streaming pass, as adam_dual_kernel"),
    # the wide hidden sizes (512 / 1024) of CDAE on list batches
    (r"void yr::cdae_sampled_decode_kernel<64, (8|16), true, (true|false)>", 128, 34 * 1024,
     "a wave per position, two W_o rows of 8 / 16 registers in flight beside z and dz: four waves per SIMD "
     "(512 / 4 -> 128) = four workgroups per CU, 4 x 33 KB of 160 KB LDS (staged list 16 KB + 4 x H floats of dz)"),
    (r"void yr::cdae_hidden_bwd_dwh_t_kernel<(2|4)>", 64, 17 * 1024,
     "up to four hidden units per thread in registers: eight waves per SIMD (512 / 8 -> 64), the staged list in LDS"),
    (r"void yr::adam_flat_kernel<(true|false), true>", 64, 1024,
     "streaming pass with a barrier per chunk for marked rows of 512 / 1,024 floats: eight waves per SIMD, as the plain form"),
    # S3Rec scoring: the LDS tiles are dynamic (13 KB at E = 16, L <= 32 up to 146 KB at E = 128, L > 32), none static
    (r"void yr::s3rec_encode_kernel<(16|32|64|128), false>", 256, 1024,
     "a workgroup per sequence, LDS-bound: one to two workgroups of four waves per CU at the reference's shapes "
     "(81.5 KB at E = 64, L = 50), so two waves per SIMD (512 / 2 -> 256) is all the registers have to allow"),
    (r"yr::s3rec_scores_kernel", 64, 0, "16 lanes per dot product, streaming: eight waves per SIMD"),
    (r"void yr::s3rec_encode_kernel<(16|32|64|128), true>", 256, 1024,
     "S3Rec training forward: a workgroup per sequence and LDS-bound like the scoring encoder, two waves per SIMD"),
    (r"void yr::s3rec_backward_kernel<(16|32|64|128)>", 512, 1024,
     "S3Rec backward: the same tiles plus one row of floats; at the reference's shape (81.7 KB at E = 64, L = 50) LDS "
     "admits one workgroup per CU, so one wave per SIMD (512 registers) costs nothing there; no scratch"),
    (r"yr::s3rec_(score_grad|item_partials|item_combine)_kernel", 64, 0,
     "element-wise pass and the two ordered passes of the item gradient: eight waves per SIMD"),
    (r"void yr::s3rec_cbce_kernel<(16|32|64), (true|false)>", 256, 9 * 1024,
     "S3Rec pre-training, catalogue BCE: the owned rows (E / 2 registers) and their gradient (E / 2) stay in registers "
     "beside one tile of logits; two workgroups per CU = two waves per SIMD (512 / 2 -> 256)"),
    (r"void yr::s3rec_cbce_kernel<128, (true|false)>", 512, 17 * 1024,
     "as above at E = 128: 64 + 64 row registers, one wave per SIMD; 16.1 KB of LDS for the wave-order sum; no scratch"),
    (r"yr::s3rec_cbce_(reduce|loss)_kernel", 64, 3 * 1024, "streaming sums in a fixed order"),
    (r"void yr::s3rec_rank_kernel<(16|32|64)>", 128, 1024,
     "S3Rec full-catalogue rank: the owned rows (E / 2 registers) beside one tile of scores and nothing else, so "
     "four waves per SIMD (512 / 4 -> 128): more than the two workgroups per CU of the cbce kernel; no scratch"),
    (r"void yr::s3rec_rank_kernel<128>", 256, 1024, "as above at E = 128: 64 row registers, two waves per SIMD"),
    (r"yr::s3rec_rank_sum_kernel", 64, 0, "streaming integer sums of the chunks' counts"),
    # MF / NGCF ranks of every held-out item (csrc/catalogue_rank.hip; figures in profiles/catalogue_rank_resources.txt)
    (r"void yr::cr_sweep_kernel<(16|32|64), (true|false)>", 168, 7 * 1024,
     "catalogue ranks: s3rec_rank_kernel's tile beside the slot's best / worst target and the binary search's "
     "cursor; the 32 slots' sorted lists and integer bins in LDS (3 x 32 x 17 words); at least three waves per SIMD "
     "(512 / 3 -> 168; 128 / 130 at D = 64); no scratch"),
    (r"void yr::cr_sweep_kernel<128, (true|false)>", 256, 7 * 1024,
     "as above at D = 128: 64 row registers (one table) or a layer's 64 at a time, two waves per SIMD"),
    (r"void yr::cr_targets_kernel<(16|32|64|128), (true|false)>", 168, 5 * 1024,
     "the targets' scores from the sweep's tile function and the rank sort of the slots' lists (2 x 32 x 17 words)"),
    (r"yr::cr_(slots|finish)_kernel", 64, 2 * 1024, "integer scan of the rows' slot counts; integer sums of the bins"),
    (r"yr::metrics_from_ranks(_sum|_finalize)?_kernel", 96, 2 * 1024,
     "a wave per user over its ranks, float64 sums in a fixed order; the per-k columns live in dynamic LDS"),
    # CDAE without negative sampling: the catalogue BCE on the geometry of s3rec_cbce_kernel
    (r"void yr::cdae_cbce_kernel<(16|32|64), (true|false)>", 256, 9 * 1024,
     "CDAE plain BCE, catalogue sweep: the owned rows (H / 2 registers), their gradient (H / 2) and one tile of "
     "pre-activations, with expf / logf / the division of the dense decoder's epilogue; two workgroups per CU = two "
     "waves per SIMD (512 / 2 -> 256; 230 at H = 64 owning rows); no scratch"),
    (r"void yr::cdae_cbce_kernel<128, (true|false)>", 512, 17 * 1024,
     "as above at H = 128: 64 + 64 row registers, one wave per SIMD; 16.1 KB of LDS for the wave-order sum; no scratch"),
    (r"yr::cdae_cbce_reduce_kernel", 64, 0, "streaming sums of the chunks' partials in a fixed order"),
    # CDAE list-batch step, reproducible form (csrc/cdae_owned.hip; figures in profiles/cdae_owned_resources.txt)
    (r"void yr::cdae_owned_decode_kernel<(32|64), (4|8|16), (true|false)>", 128, 34 * 1024,
     "the default decoder's geometry and budget: four waves per SIMD, the staged list + the groups' dz rows in LDS"),
    (r"void yr::cdae_owned_gather_kernel<(1|2|4|8|16), (true|false)>", 96, 0,
     "a column owner keeps H / lanes accumulators and one row of the operand: five waves per SIMD at 16 floats per lane"),
    (r"yr::cdae_owned_(count|sum_splits|hidden_rows|hidden_sums)_kernel", 64, 2 * 1024,
     "integer counting sort and streaming row passes: eight waves per SIMD"),
    (r"void yr::owned_scan_kernel<(true|false)>", 64, 1024,
     "the tiled integer scan of the owner passes (owned_scan.h; CDAE and NGCF): eight waves per SIMD"),
    # NGCF fused step, reproducible form (csrc/ngcf_owned.hip; figures in profiles/ngcf_owned_resources.txt)
    (r"void yr::ngcf_owned_score_bwd_kernel<(16|32|64|128), (true|false)>", 64, 0,
     "a lane group per row, one accumulator and four contributions' rows ahead: eight waves per SIMD to hide the "
     "three dependent loads per contribution"),
    (r"yr::ngcf_owned_(count|fill|rank|dw_reduce)_kernel", 64, 0,
     "integer counting sort, the rank pass and the slot sum (eight slots' loads in flight): eight waves per SIMD"),
    (r"void yr::ngcf_owned_dw_slots_kernel<(16|32|64), (true|false)>", 176, 48 * 1024,
     "ngcf_dense_bwd_weight_kernel with a store epilogue: the same body, so the same registers and 48 KB of LDS"),
    (r"void yr::ngcf_owned_dw_slots_kernel<128, (true|false)>", 512, 48 * 1024,
     "as above at D = 128: 8 output tiles per wave (128 accumulators), one wave per SIMD as the default kernel"),
    # DCN training step, reproducible form (csrc/dcn_owned.hip; figures in profiles/dcn_owned_resources.txt)
    (r"yr::dcn_head_kernel", 200, 38916,
     "the default head: exactly what it compiled to before the ordered form shared its row loop (dcn_head_rows.h)"),
    (r"yr::dcn_head_ordered_kernel", 256, 1024,
     "the same row loop with a private accumulator per wave in DYNAMIC LDS (up to 155,664 B: one workgroup per CU at the "
     "largest shape, five at the default one), so two waves per SIMD (512 / 2 -> 256) is all the registers have to allow"),
    (r"yr::dcn_(head_reduce|owned_chunk|owned_attr_rows)_kernel", 64, 0,
     "streaming sums in a fixed order, eight or sixteen loads ahead of their adds: eight waves per SIMD"),
    (r"yr::dcn_owned_rows_kernel", 96, 0,
     "a lane group per touched row, four entries' dx rows (three float4 each on an item row) ahead of their adds: five "
     "waves per SIMD"),
]
# Scratch (spilled registers) per lane.  The forms the benchmark and the trainers run by default — width 64, summation
# order free — must have none; the deterministic-order forms and some forms of the other widths are held at 64 VGPRs by
# __launch_bounds__ and spill a few words (measured cost in profiles/r02_deterministic_mode_cost.txt) — capped here
# so that it cannot grow unnoticed.
SCRATCH_ALLOWED = {
    r"void yr::owner_pass_kernel<(16|32|64|128), (true|false), (true|false), true, [01]>": 64,   # deterministic order
    r"void yr::owner_pass_kernel<(16|32|128), (true|false), (true|false), false, [01]>": 16,
    r"void yr::topk_masked_kernel<32, 1024>": 160,       # unfused fallback for 16 < k <= 32 (a 32-entry list per thread)
}


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.strip().split("\n")


def _write_isa(isa_dir, obj, dis):
    """One file per symbol of the disassembly: instructions and branch targets (symbol + offset), no addresses or
    encodings — text that stays the same when a kernel merely moves inside its code object."""
    os.makedirs(isa_dir, exist_ok=True)
    out = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if out:
                out.close()
            sym = m.group(1)          # mangled names can exceed a file name: cut, and keep them apart by a digest
            out = open(os.path.join(isa_dir, f"{os.path.basename(obj)}.{sym[:120]}.{hashlib.sha1(sym.encode()).hexdigest()[:8]}.s"), "w")
            out.write(f"<{sym}>:\n")
        elif out and line.strip():
            out.write(re.sub(r"\s*// [0-9A-F]+:( [0-9A-F]{8})+", "", line) + "\n")
    if out:
        out.close()


def read_object(obj, isa_dir=None):
    """{demangled kernel name: dict(vgpr, agpr, sgpr, lds, scratch, spill)} of one .o (gfx950 bundle)."""
    tmp = tempfile.mkdtemp(prefix="yr_kres.")
    try:
        local = os.path.join(tmp, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], cwd=tmp, capture_output=True, check=True)
        cos = [f for f in glob.glob(local + ".*") if "gfx950" in f]
        if not cos:
            return {}
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", cos[0]], capture_output=True, text=True, check=True).stdout
        # scratch instructions per kernel symbol (a private segment can be RESERVED without ever being accessed:
        # what matters is scratch traffic)
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", cos[0]], capture_output=True, text=True,
                             check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if isa_dir:
        _write_isa(isa_dir, obj, dis)
    kernels, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s+(-\s+)?\.(\w+):\s+(.*)$", line)
        if not m:
            continue
        dash, key, val = m.groups()
        if key == "agpr_count" and dash:                   # first key of a kernel entry
            cur = {}
            kernels.append(cur)
        if cur is not None and key in ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                       "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "name"):
            cur[key] = val.strip()
    kernels = [k for k in kernels if "name" in k]
    scratch_ops, sym = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            scratch_ops[sym] = 0
        elif sym and re.search(r"\bscratch_(load|store)", line):
            scratch_ops[sym] += 1
    names = _demangle([k["name"] for k in kernels]) if kernels else []
    return {n: dict(vgpr=int(k["vgpr_count"]), agpr=int(k["agpr_count"]), sgpr=int(k["sgpr_count"]),
                    lds=int(k["group_segment_fixed_size"]), scratch=int(k["private_segment_fixed_size"]),
                    spill=int(k.get("vgpr_spill_count", 0)), scratch_ops=scratch_ops.get(k["name"], 0))
            for n, k in zip(names, kernels)}


def read_all(isa_dir=None):
    out = {}
    for obj in sorted(glob.glob(os.path.join(CSRC, "*.o"))):
        for name, r in read_object(obj, isa_dir).items():
            r["file"] = os.path.basename(obj)
            out[name] = r
    return out


def check(kernels=None):
    """Raise RuntimeError listing every kernel over its budget; returns the kernel table."""
    kernels = read_all() if kernels is None else kernels
    if not kernels:
        raise RuntimeError("no gfx950 kernels found in the built objects (run make first)")
    bad = []
    for pat, max_vgpr, max_lds, why in BUDGETS:
        hit = [(n, r) for n, r in kernels.items() if re.match(pat, n)]
        if not hit:
            bad.append(f"budget pattern matches no kernel (renamed?): {pat}")
        for n, r in hit:
            if r["vgpr"] > max_vgpr or (max_lds and r["lds"] > max_lds):
                bad.append(f"{n[:100]}: {r['vgpr']} VGPRs / {r['lds']} B LDS over the budget of {max_vgpr} / {max_lds} ({why})")
    for n, r in kernels.items():
        allowed = max([v for p, v in SCRATCH_ALLOWED.items() if re.match(p, n)], default=0)
        # a reserved private segment that no instruction touches (scratch_ops == 0, no spilled VGPR) is not traffic
        used = r["scratch"] if (r.get("scratch_ops", 1) > 0 or r["spill"] > 0) else 0
        if used > allowed or (allowed == 0 and r["spill"] > 0):
            bad.append(f"{n[:100]}: {r['scratch']} B of scratch per lane, {r['spill']} spilled VGPRs, {r.get('scratch_ops', '?')} scratch instructions (spills are never acceptable on this path)")
    if bad:
        raise RuntimeError("kernel resource budgets exceeded:\n  " + "\n  ".join(bad))
    return kernels


if __name__ == "__main__":
    ks = read_all(sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--isa" else None)
    for n, r in sorted(ks.items(), key=lambda kv: (kv[1]["file"], kv[0])):
        print(f"{r['file']:18s} vgpr {r['vgpr']:3d} agpr {r['agpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']:4d} ({r['scratch_ops']:2d} ops)  {n[:110]}")
    try:
        check(ks)
        print(f"{len(ks)} kernels, all budgets met")
    except RuntimeError as e:
        print(e)
        sys.exit(1)
