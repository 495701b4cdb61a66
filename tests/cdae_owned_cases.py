"""Cases and generators for the owner-pass kernels of csrc/cdae_owned.hip (tests/test_gpu_cdae_owned_edges.py runs them
on the GPU, tests/test_cdae_owned_host.py shows without one that every case reaches the loop end it is there for and
that the bars notice a lost or doubled entry).  Importable helper, no fixtures; the float64 reference and the bars are
those of cdae_ref64.py.  Two things are added to its inputs:

  heavy columns     40 columns (every column when the catalogue has fewer) that are a loss position AND an encoder entry
                    of every batch row: column 0, column I - 1, both sides of the first sub-list boundary, the rest
                    spread evenly — a column owner then walks as many entries as the batch has rows;
  order-sensitive   row r of z and of dz scaled by 2^((7 r mod 21) - 10), W_o by 2^-10 (sigmoid output: every
                    pre-activation stays within +-3, everything finite): an f32 sum over the rows then depends on its
                    order in most elements, so "two calls agree bit for bit" says something.
"""
import numpy as np

import cdae_ref64 as R

PARTS = 32                        # kListParts
N_HEAVY = 40
NUM_USERS = 50
SENTINEL = np.float32(-7777.0)
GUARD = 64
KEPT = np.float32(0.25)           # what the rows a call must not touch hold before it


def cpp_of(I):
    """yr_cdae_sparse_part_columns: columns per sub-list."""
    return ((I + PARTS - 1) // PARTS + 3) // 4 * 4


def splits_of(B):
    """yr_cdae_sampled_decode_splits."""
    return max(1, min(8, 512 // B)) if B > 0 else 1


def workspace_bytes(B, I, H):
    """yr_cdae_owned_workspace_bytes: the counts and cursors [2 I] and the segment starts [I + 1] (int32), row and value of every
    list slot (B 32 cpp of each), B splits H floats of dz partials / dz'; every part rounded up to 16 bytes."""
    up = lambda b: (b + 15) // 16 * 16
    entries = B * PARTS * cpp_of(I)
    return up(8 * I) + up(4 * (I + 1)) + 2 * up(4 * entries) + up(4 * B * H * splits_of(B))


def heavy_columns(I):
    if I <= N_HEAVY:
        return np.arange(I)
    cpp = cpp_of(I)
    must = {0, I - 1, cpp - 1, cpp}
    rest = [int(c) for c in np.linspace(1, I - 2, 3 * N_HEAVY).astype(int) if int(c) not in must]
    cols, k = set(must), 0
    while len(cols) < N_HEAVY:
        cols.add(rest[k]); k += 1
    return np.array(sorted(cols), np.int64)


def row_scales(B):
    return (2.0 ** ((7 * np.arange(B)) % 21 - 10)).astype(np.float32)


# what a case is there for, checked by test_cdae_owned_host.test_every_case_reaches_its_loop_end:
#   col_rows   >= rows in the fullest column of both lists          row_len  >= entries in the longest row of both lists
#   splits     workgroups per row of the decoder                    lanes, epl  column-owner geometry (H / epl lanes)
def _case(id, B, I, H, oact=1, hact=1, with_bo=True, heavy=False, long=False, users="plain", order=False, **reach):
    return dict(id=id, B=B, I=I, H=H, oact=oact, hact=hact, with_bo=with_bo, heavy=heavy, long=long, users=users,
                order=order, reach=reach)


def kernel_cases():
    I2 = 9                        # = 2 cpp(9) + 1: two full sub-lists of four columns and one column in the third
    assert I2 == 2 * cpp_of(I2) + 1
    cases = [
        _case("one_of_everything", 1, 1, 16, heavy=True, col_rows=1, row_len=1, splits=8, lanes=16, epl=1),
        _case("B31", 31, 33, 32, heavy=True, oact=0, col_rows=31, splits=8, lanes=32, epl=1),
        _case("B32", 32, 33, 32, heavy=True, hact=0, col_rows=32, splits=8, lanes=32, epl=1),
        _case("B33", 33, 33, 32, heavy=True, with_bo=False, col_rows=33, splits=8, lanes=32, epl=1),
        _case("sublist_edges_H128", 65, I2, 128, heavy=True, oact=0, col_rows=65, splits=7, lanes=64, epl=2),
        _case("sublist_edges_H256", 65, I2, 256, heavy=True, col_rows=65, splits=7, lanes=64, epl=4),
        _case("wave_per_position_H512", 5, 300, 512, heavy=True, oact=0, with_bo=False, col_rows=5, splits=8, lanes=64, epl=8),
        _case("wave_per_position_H1024", 5, 300, 1024, heavy=True, col_rows=5, splits=8, lanes=64, epl=16),
        _case("column_past_a_workgroup", 300, 300, 64, heavy=True, col_rows=257, splits=1, lanes=64, epl=1),
        _case("column_past_1024_rows", 1025, 200, 16, heavy=True, hact=0, col_rows=1025, splits=1, lanes=16, epl=1),
        _case("two_splits", 256, 300, 64, heavy=True, oact=0, col_rows=256, splits=2, lanes=64, epl=1),
        _case("long_rows_H16", R.N_LONG, R.I_LONG, 16, long=True, row_len=R.I_LONG, splits=8, lanes=16, epl=1),
        _case("long_rows_H512", R.N_LONG, R.I_LONG, 512, long=True, oact=0, hact=0, row_len=R.I_LONG, splits=8, lanes=64, epl=8),
        _case("duplicate_users", 12, 77, 64, users="duplicates", heavy=True, col_rows=12, splits=8, lanes=64, epl=1),
        _case("identity_no_bias", 40, 120, 32, oact=0, with_bo=False, splits=8, lanes=32, epl=1),
        _case("sigmoid_no_bias", 40, 120, 32, oact=1, with_bo=False, splits=8, lanes=32, epl=1),
        _case("identity_bias", 40, 120, 32, oact=0, with_bo=True, splits=8, lanes=32, epl=1),
        _case("order_sensitive", 300, 200, 64, heavy=True, order=True, col_rows=300, splits=1, lanes=64, epl=1),
    ]
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


def case(id):
    return next(c for c in kernel_cases() if c["id"] == id)


def gen(c, seed=0, heavy=None):
    """The inputs of one case: decoder side (target, negmask, z, Wo, bo), hidden side (x_in, dz, zh, user) — the two
    entry points are run independently, each on generated inputs.  ``heavy`` overrides the case's heavy-column flag
    (the left-over check runs a batch without them on the same shape)."""
    B, I, H = c["B"], c["I"], c["H"]
    rs = np.random.RandomState(9000 + 31 * seed + B + 7 * I + 3 * H + c["oact"])
    if c["long"]:
        target, negmask = R.loss_rows(rs, I, R.LOSS_COUNTS)
        x = R.input_rows(rs, I, R.ENC_COUNTS)
    else:
        hi = min(I, 40) + 1
        target, negmask = R.loss_rows(rs, I, [int(k) for k in rs.randint(0, hi, B)])
        x = R.input_rows(rs, I, [int(k) for k in rs.randint(0, min(I, 30) + 1, B)])
    hc = heavy_columns(I) if (c["heavy"] if heavy is None else heavy) else np.zeros(0, np.int64)
    if len(hc):
        free = (target[:, hc] + negmask[:, hc]) == 0
        pos = rs.rand(B, len(hc)) < 1.0 / 6.0
        target[:, hc] = np.where(free & pos, 1.0, target[:, hc])
        negmask[:, hc] = np.where(free & ~pos, 1.0, negmask[:, hc])
        x[:, hc] = np.where(x[:, hc] == 0, (0.5 + rs.rand(B, len(hc))).astype(np.float32), x[:, hc])
    z, Wo, bo = R.decoder_params(rs, B, H, I, c["oact"], c["with_bo"])
    dz, zh, user = R.hidden_inputs(rs, B, H, NUM_USERS)
    if c["users"] == "duplicates":                     # three rows of one user, not adjacent; both out-of-range ends
        user[:] = rs.permutation(NUM_USERS)[:B]
        user[[0, 2, B - 1]] = user[0]
        user[1], user[3] = -1, NUM_USERS
    if c["order"]:
        assert c["oact"] == 1
        s = row_scales(B)[:, None]
        z, dz = z * s, dz * s
        Wo = (Wo * np.float32(2.0 ** -10)).astype(np.float32)
    return dict(target=target, negmask=negmask, z=z, Wo=Wo, bo=bo, x=x, dz=dz, zh=zh, user=user, heavy=hc,
                partials_in=rs.rand(B * splits_of(B)).astype(np.float32))


def reference(c, g, weight=None, x=None):
    """(decoder outputs, hidden outputs) of cdae_ref64 for the generated inputs; the hidden side scales dz by the
    decoder's position count, as a training step does."""
    S = splits_of(c["B"])
    dec = R.sampled_decode(g["z"], g["Wo"], g["bo"], g["target"], g["negmask"], c["oact"], weight=weight, splits=S)
    hid = R.hidden_bwd(g["dz"], g["zh"], c["hact"], g["user"], dec["count"], g["x"] if x is None else x, NUM_USERS)
    return dec, hid


def reached(c, g):
    """The figures a case's ``reach`` entries are checked against."""
    sel, xe = (g["target"] + g["negmask"]) != 0, g["x"] != 0
    H = c["H"]
    epl = 1 if H <= 64 else H // 64
    return dict(col_rows=int(min(sel.sum(0).max(), xe.sum(0).max())), row_len=int(min(sel.sum(1).max(), xe.sum(1).max())),
                splits=splits_of(c["B"]), lanes=H // epl, epl=epl)
