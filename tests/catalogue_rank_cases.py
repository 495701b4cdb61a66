"""Cases for the catalogue rank sweep (engine.catalogue_ranks), shared by test_catalogue_rank_host.py — which asserts
that every case reaches the loop end it is named for (``plan``) — and test_gpu_catalogue_rank.py.

EXACT cases: tables of integers in [-3, 3] (catalogue_rank_ref64.certify_exact), so every score is an integer, ties are
everywhere and the id decides them; a correct kernel equals float64 exactly.  Each case mixes, row by row:
  * target counts 0, 1, CAP - 1, CAP, CAP + 1, 2 CAP + 1 (as far as the catalogue allows): no slot, one slot short /
    full, two slots with one entry in the second, three slots;
  * targets on the first and last item of a 32-item tile and of a 2,048-item chunk, and the catalogue's last item;
  * mask rows: empty; all items but one; ending exactly on a tile end; random with one of the row's targets masked;
    random without a target;
  * item rows copied onto both neighbours of a target (the id decides in both directions);
  * the last row repeats the first row's user id, targets and masks (equal ranks).
``zero=True``: all-zero tables, every score ties.
"""
import numpy as np

import catalogue_rank_ref64 as ref

CAP, TILE, CHUNK = ref.CAP, ref.TILE, ref.CHUNK
TARGET_COUNTS = (0, 1, CAP - 1, CAP, CAP + 1, 2 * CAP + 1)

# (D, L, N, items): every width with every layer count of {1, 2, 3, 8}; every N of {1, 31, 32, 33, 65}; every
# catalogue of {1, 31, 32, 33, 2047, 2048, 2049, 4097}
EXACT_SPECS = [
    (16, 1, 1, 1), (16, 2, 31, 31), (16, 3, 32, 32), (16, 8, 33, 33),
    (32, 1, 65, 2047), (32, 2, 33, 2048), (32, 3, 31, 2049), (32, 8, 32, 4097),
    (64, 1, 33, 4097), (64, 2, 65, 33), (64, 3, 65, 2049), (64, 8, 1, 2048),
    (128, 1, 32, 2049), (128, 2, 31, 4097), (128, 3, 33, 2047), (128, 8, 65, 32),
]


def spec_id(spec):
    return "D{}-L{}-N{}-I{}".format(*spec)


class Case:
    pass


def special_items(items):
    """First / last item of a tile and of a chunk, and the catalogue's last item."""
    s = [0, TILE - 1, TILE, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, items - 1, items - TILE]
    return [x for x in dict.fromkeys(s) if 0 <= x < items]


_BUILT = {}


def build_exact(spec, zero=False):
    key = (spec, zero)
    if key in _BUILT:
        return _BUILT[key]
    D, L, N, items = spec
    rs = np.random.RandomState(1000 + 13 * D + 7 * L + 3 * N + items)
    nu = N + 3
    gen = (lambda shape: np.zeros(shape, np.float32)) if zero else \
        (lambda shape: rs.randint(-3, 4, shape).astype(np.float32))
    c = Case()
    c.D, c.L, c.N, c.items, c.num_users = D, L, N, items, nu
    c.layers_user = [gen((nu, D)) for _ in range(L)]
    c.layers_item = [gen((items, D)) for _ in range(L)]
    c.users = rs.randint(0, nu, N).astype(np.int64)
    special = special_items(items)
    c.pos, c.masks, c.mask_kind = [], [], []
    for r in range(N):
        want = TARGET_COUNTS[(r + L) % len(TARGET_COUNTS)]
        count = min(want, items)
        first = [x for x in rs.permutation(special)][:count]
        rest = [x for x in rs.permutation(items) if x not in set(first)][:count - len(first)]
        tg = [int(x) for x in rs.permutation(first + rest)]
        kind = ("empty", "all_but_one", "tile_end", "masked_target", "random")[(r + D // 16) % 5]
        if kind == "empty":
            m = []
        elif kind == "all_but_one":
            keep = tg[0] if tg else items - 1
            m = [x for x in range(items) if x != keep]
        elif kind == "tile_end":
            end = min(items, TILE * (1 + r % 3)) - 1          # the last masked id closes a tile (or the catalogue)
            m = sorted(set(rs.choice(end + 1, min(end + 1, 5), replace=False).tolist() + [end]))
        elif kind == "masked_target":
            m = sorted(set(rs.choice(items, min(items, 9), replace=False).tolist() + tg[:1]))
        else:
            m = sorted(set(rs.choice(items, min(items, 9), replace=False).tolist()) - set(tg))
        c.pos.append(tg)
        c.masks.append([int(x) for x in m])
        c.mask_kind.append(kind)
    # duplicate item rows on both sides of a target of the first rows with an unmasked target away from the ends
    c.dups = []
    taken = set()
    for r in range(N):
        for t in c.pos[r]:
            if 0 < t < items - 1 and not ({t - 1, t, t + 1} & taken) and len(c.dups) < 4:
                for I in c.layers_item:
                    I[t - 1] = I[t]
                    I[t + 1] = I[t]
                taken |= {t - 1, t, t + 1}
                c.dups.append((r, t))
                break
    if N >= 2:                                               # a user id repeated, with the same lists
        c.users[N - 1] = c.users[0]
        c.pos[N - 1] = list(c.pos[0])
        c.masks[N - 1] = list(c.masks[0])
        c.mask_kind[N - 1] = c.mask_kind[0]
    ref.certify_exact(c.layers_user, c.layers_item)
    c.pos_ptr, c.pos_idx = ref.csr(c.pos)
    c.mask_ptr, c.mask_idx = ref.csr(c.masks)
    S, _ = ref.scores64(c.layers_user, c.layers_item, c.users)
    c.S = S
    c.rank = ref.ranks(S, c.masks, c.pos)
    c.score = np.array([S[r, t] for r in range(N) for t in c.pos[r]], np.float64)
    _BUILT[key] = c
    return c


def plan(pos_lengths, items):
    """What the library makes of a call, from the constants the engine exports: slots, row tiles, column chunks, units
    (workgroups' worth of work) and whether the grid loop runs (more units than one launch's workgroups)."""
    slots = sum(-(-n // CAP) for n in pos_lengths)
    tiles = -(-slots // TILE)
    chunks = -(-items // CHUNK)
    return dict(slots=slots, tiles=tiles, chunks=chunks, units=tiles * chunks, loops=tiles * chunks > ref.GRID_MAX,
                col_tiles=-(-items // TILE), ragged_tile=items % TILE != 0, ragged_slots=slots % TILE != 0)


# ---- the grid loop: more units than one launch's workgroups, in a narrow and cheap shape ----
GRID_ROWS = TILE * ref.GRID_MAX + 1          # one target each: 2,049 row tiles x 1 chunk
GRID_D, GRID_ITEMS = 16, 8


def build_grid():
    rs = np.random.RandomState(5)
    c = Case()
    c.num_users, c.items, c.D = 257, GRID_ITEMS, GRID_D
    c.U = rs.randint(-3, 4, (c.num_users, GRID_D)).astype(np.float32)
    c.I = rs.randint(-3, 4, (GRID_ITEMS, GRID_D)).astype(np.float32)
    c.users = rs.randint(0, c.num_users, GRID_ROWS).astype(np.int64)
    c.targets = rs.randint(0, GRID_ITEMS, GRID_ROWS).astype(np.int64)
    c.masked = ((c.targets + 1 + rs.randint(0, GRID_ITEMS - 1, GRID_ROWS)) % GRID_ITEMS).astype(np.int64)  # != target
    return c


# ---- random f32 inputs: ranks inside the float64 interval ----
# (D, L, N, items, m): m = non-zero dims per item row over all L D (0: dense)
RANDOM_SPECS = [(16, 1, 40, 4200, 0), (32, 3, 40, 2100, 4), (64, 2, 70, 2100, 4), (128, 1, 40, 1100, 4),
                (64, 8, 33, 300, 4),
                # dense rows beyond W = 16, the catalogue as small as the estimate in build_random's docstring asks:
                # items x c_bound(W) x 0.64 sqrt(W) of about 0.01 (1,100 items at W = 32, 200 at W = 128)
                (32, 1, 40, 1100, 0), (64, 2, 40, 200, 0)]
RANDOM_CAP = 0.05                            # at most this share of (row, target) pairs may have lo != hi


def build_random(spec):
    """N(0, 1) user rows; item rows N(0, 1), dense at W = L D = 16 and with m = 4 non-zero dims beyond.  The bar of a
    score is c_bound(W) A with A = sum |products|, and two scores s_t, s_i are told apart when they differ by more than
    e_t + e_i: a target has about  items x c_bound(W) x A / spread  undecided neighbours, A / spread = 0.64 sqrt(W)
    for dense rows (W = 512, 700 items: 0.3 per target — far over the cap) and 0.64 sqrt(m) for sparse ones (0.02).
    The cap is checked on the float64 reference alone by test_catalogue_rank_host.py."""
    key = ("random", spec)
    if key in _BUILT:
        return _BUILT[key]
    D, L, N, items, m = spec
    rs = np.random.RandomState(31 * D + L + items)
    c = Case()
    c.D, c.L, c.N, c.items, c.num_users = D, L, N, items, N + 5
    c.layers_user = [rs.standard_normal((c.num_users, D)).astype(np.float32) for _ in range(L)]
    wide = rs.standard_normal((items, L * D)).astype(np.float32)
    if m:
        keep = np.zeros((items, L * D), bool)
        for j in range(items):
            keep[j, rs.choice(L * D, m, replace=False)] = True
        wide[~keep] = 0.0
    c.layers_item = [np.ascontiguousarray(wide[:, l * D:(l + 1) * D]) for l in range(L)]
    c.users = rs.permutation(c.num_users)[:N].astype(np.int64)
    c.pos = [[int(x) for x in rs.choice(items, TARGET_COUNTS[r % len(TARGET_COUNTS)], replace=False)] for r in range(N)]
    c.masks = [sorted(int(x) for x in rs.choice(items, 25, replace=False)) if r % 3 else [] for r in range(N)]
    c.pos_ptr, c.pos_idx = ref.csr(c.pos)
    c.mask_ptr, c.mask_idx = ref.csr(c.masks)
    S, A = ref.scores64(c.layers_user, c.layers_item, c.users)
    eps = ref.bar(L, D) * A
    lo, hi = [], []
    for r in range(N):
        a, b = ref.rank_bounds_row(S[r], eps[r], c.masks[r], c.pos[r])
        lo.append(a)
        hi.append(b)
    c.lo = np.concatenate(lo + [np.zeros(0, np.int64)])
    c.hi = np.concatenate(hi + [np.zeros(0, np.int64)])
    _BUILT[key] = c
    return c
