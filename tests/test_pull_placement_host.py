"""Placement of the pull step's owner workgroups (csrc/pull_placement.h), without a GPU: the slot -> bucket map and
the item pass's start order, through the library's two host entry points (the run length G it was built with) and
through the header compiled on its own for every other run length.

    slot s = 8 j + c  ->  bucket ((j // G) * 8 + c) * G + j % G        on [0, nb rounded up to a multiple of 8 G)

Slots with equal s % 8 are the workgroups of one XCD (round-robin dispatch); they must get neighbouring buckets, and the
map must be a bijection whatever the dispatcher does."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yelprecommendation_amd", "csrc")
NBS = (1, 7, 8, 9, 63, 64, 65, 1980, 2378, 4097, 8193)
RUNS = (1, 2, 4, 8, 16, 32, 64)          # every G the header accepts up to an `off` line of 32 buckets and beyond
MAX_BUCKETS = 16383                      # kMaxBuckets

SHIM = r"""
#include "pull_placement.h"
extern "C" int run_length() { return yr::kXcdRun; }
extern "C" int owner_bucket(int slot, int nb) {
  if (nb <= 0 || slot < 0 || slot >= yr::owner_slots(nb)) return -2;
  const int k = yr::owner_bucket(slot);
  return k < nb ? k : -1;
}
extern "C" int start_order(const double* load, int nb, int32_t* out) { yr::owner_start_order(load, nb, out); return 0; }
"""


class Placement:
    def __init__(self, bucket_fn, order_fn, G=None):
        self._bucket, self._order = bucket_fn, order_fn
        # G as the map shows it: slot 8 j is bucket j while j < G, and 8 G at j = G
        self.G = G if G is not None else next(j for j in range(1, 1025) if bucket_fn(8 * j, MAX_BUCKETS) != j)

    def slots(self, nb):
        r = 8 * self.G
        return -(-nb // r) * r

    def buckets(self, nb):
        """bucket of every slot (-1: none)"""
        return np.array([self._bucket(s, nb) for s in range(self.slots(nb))], np.int64)

    def classes(self, nb):
        """class (slot % 8) of every bucket"""
        b = self.buckets(nb)
        s = np.flatnonzero(b >= 0)
        cls = np.full(nb, -1, np.int64)
        cls[b[s]] = s % 8
        return cls

    def order(self, load):
        load = np.ascontiguousarray(load, np.float64)
        out = np.full(load.shape[0], -7, np.int32)
        assert self._order(load.ctypes.data, load.shape[0], out.ctypes.data) == 0
        return out.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _library():
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    return Placement(lib.yr_bpr_mf_pull_owner_bucket, lib.yr_bpr_mf_pull_item_start_order)


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    """The header compiled for the host with every run length: {G: Placement}"""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler to build pull_placement.h with"
    d = tmp_path_factory.mktemp("placement")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    out = {}
    for G in RUNS:
        so = d / f"shim_g{G}.so"
        subprocess.run([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", f"-DYR_XCD_RUN={G}", f"-I{CSRC}", str(src), "-o", str(so)],
                       check=True)
        lib = ctypes.CDLL(str(so))
        lib.start_order.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        assert lib.run_length() == G
        out[G] = Placement(lib.owner_bucket, lib.start_order, G)
    return out


def _formula(s, G):
    c, j = s % 8, s // 8
    return ((j // G) * 8 + c) * G + j % G


def _check_map(pl, nb):
    G = pl.G
    b = pl.buckets(nb)
    assert b.shape[0] % (8 * G) == 0 and 0 <= b.shape[0] - nb < 8 * G
    want = np.array([_formula(s, G) for s in range(b.shape[0])])
    assert np.array_equal(np.sort(want), np.arange(b.shape[0])), "the formula itself is a bijection of the padded space"
    assert np.array_equal(b, np.where(want < nb, want, -1))
    assert np.array_equal(np.sort(b[b >= 0]), np.arange(nb)), "every bucket has exactly one slot"
    # neighbours: slot s + 8 is the next bucket of the run, or the first of the class's next run (8 G further on)
    for s in range(b.shape[0] - 8):
        k0, k1 = want[s], want[s + 8]
        assert 0 < k1 - k0 < G or k1 == (k0 // G) * G + 8 * G, (s, k0, k1)
    # every run of G buckets lies in one class
    cls = pl.classes(nb)
    assert cls.min() >= 0
    for r0 in range(0, nb, G):
        assert len(set(cls[r0:r0 + G])) == 1, (r0, cls[r0:r0 + G])
    assert np.array_equal(cls, (np.arange(nb) // G) % 8)


@pytest.mark.parametrize("nb", NBS)
def test_library_slot_map_is_a_permutation(nb):
    pl = _library()
    assert pl.G in RUNS
    _check_map(pl, nb)


def test_library_entry_points_check_their_arguments():
    from yelprecommendation_amd import _lib
    lib = _lib.load()
    pl = _library()
    assert lib.yr_bpr_mf_pull_owner_bucket(-1, 9) == -2 and lib.yr_bpr_mf_pull_owner_bucket(0, 0) == -2
    assert lib.yr_bpr_mf_pull_owner_bucket(pl.slots(9), 9) == -2 and lib.yr_bpr_mf_pull_owner_bucket(0, MAX_BUCKETS + 1) == -2
    assert lib.yr_bpr_mf_pull_owner_bucket(0, 1) == 0 and lib.yr_bpr_mf_pull_owner_bucket(1, 1) == -1
    out = np.zeros(4, np.int32)
    load = np.array([1.0, np.nan, 2.0, 0.0])
    assert lib.yr_bpr_mf_pull_item_start_order(None, 4, out.ctypes.data) == -2
    assert lib.yr_bpr_mf_pull_item_start_order(load.ctypes.data, 4, None) == -2
    assert lib.yr_bpr_mf_pull_item_start_order(load.ctypes.data, 0, out.ctypes.data) == -2
    assert lib.yr_bpr_mf_pull_item_start_order(load.ctypes.data, 4, out.ctypes.data) == -2          # NaN
    assert not out.any()


@pytest.mark.parametrize("G", RUNS)
def test_slot_map_for_every_run_length(shims, G):
    for nb in NBS:
        _check_map(shims[G], nb)


def test_library_agrees_with_the_header_at_its_run_length(shims):
    pl, twin = _library(), shims[_library().G]
    for nb in (9, 65, 2378):
        assert np.array_equal(pl.buckets(nb), twin.buckets(nb))
        load = np.random.RandomState(nb).rand(nb)
        assert np.array_equal(pl.order(load), twin.order(load))


def _check_order(pl, load, tag):
    nb = load.shape[0]
    order = pl.order(load)
    assert np.array_equal(np.sort(order), np.arange(nb)), (tag, "a permutation")
    cls = pl.classes(nb)
    for c in range(8):
        mine = order[cls[order] == c]                  # the class's buckets in the order they start
        assert np.all(np.diff(load[mine]) <= 0), (tag, c, "heaviest first inside a class")
        assert np.array_equal(mine, mine[np.argsort(-load[mine], kind="stable")]), (tag, c, "equal loads by index")
    full = 8 * int(np.bincount(cls, minlength=8).min())
    s = np.arange(full)
    assert np.array_equal(cls[order[s]], s % 8), (tag, "slot s starts a bucket of class s % 8 while every class has one")
    # once a class is used up its slots take the heaviest bucket left over
    used = np.zeros(nb, bool)
    for s in range(nb):
        k = order[s]
        if cls[k] != s % 8:
            assert used[cls == s % 8].all(), (tag, s)
            assert load[k] == load[~used].max(), (tag, s)
        used[k] = True


@pytest.mark.parametrize("nb", (1, 7, 8, 9, 64, 65, 1980, 2378, 2384))
def test_library_start_order(nb):
    pl = _library()
    rs = np.random.RandomState(nb)
    _check_order(pl, rs.rand(nb), f"random {nb}")
    _check_order(pl, rs.zipf(1.3, nb).astype(np.float64), f"zipf with ties {nb}")
    _check_order(pl, np.full(nb, 3.0), f"all equal {nb}")


@pytest.mark.parametrize("G", RUNS)
def test_start_order_for_every_run_length(shims, G):
    for nb in (9, 64, 65, 2378):
        rs = np.random.RandomState(nb + G)
        _check_order(shims[G], rs.rand(nb), f"G={G} random {nb}")
        _check_order(shims[G], np.ones(nb), f"G={G} all equal {nb}")


def test_step_uses_the_builder():
    """BPRMFStep.set_item_order takes its order from the builder (source check: the call needs a GPU tensor)."""
    src = open(os.path.join(ROOT, "yelprecommendation_amd", "bpr_step.py")).read()
    body = src[src.index("def set_item_order"):src.index("def _auto_item_order")]
    assert "yr_bpr_mf_pull_item_start_order" in body and "argsort" not in body
