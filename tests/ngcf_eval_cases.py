"""Certified cases for NGCF's layered evaluation sweep (engine.ngcf_eval_topk), shared by test_ngcf_eval_host.py and
test_gpu_ngcf_full_eval.py.

NGCF scores s(u, j) = sum_l E_l[u] . E_l[num_users + j]: the dot product of rows of width W = layers x D that exist in
no table.  A case is an eval_ladders case of width W (certified float64 lists, see that module) whose tables are cut
into `layers` column blocks of D: layer l is columns [l D, (l + 1) D) of case.U stacked on the same columns of case.I.
The sweep keeps one f32 accumulator per score over all W products, so eval_ladders' rounding model holds with D
replaced by W (c_bound(W)), and a correct kernel must return the certified lists exactly.

Specs (D, layers, N, rows, k) reach: a single ragged tile (N = 33); a partial wave (5 rows); one workgroup plus two
rows (130); three workgroups with a ragged last one (300); one, two and eight catalogue slices (33 / 4,100 / 16,411
items); one layer and the maximum of eight; every width; every list size (k = 1, 4, 10, 16).
"""
import numpy as np

import eval_ladders as el

SPECS = [
    (16, 2, 33, 5, 1),
    (16, 8, 4100, 300, 4),
    (32, 4, 4100, 130, 10),
    (64, 1, 4100, 130, 10),
    (64, 3, 4100, 300, 10),
    (64, 3, 16411, 300, 16),
    (64, 8, 4100, 130, 16),
    (128, 2, 16411, 130, 16),
    (128, 3, 4100, 300, 10),
    (128, 8, 33, 130, 1),
]

_BUILT = {}


def spec_id(spec):
    return "D{}-L{}-N{}-n{}-k{}".format(*spec)


def build(spec):
    """The certified case of a spec (built once per process; build_case asserts its certificate)."""
    if spec not in _BUILT:
        D, layers, N, rows, k = spec
        W = D * layers
        el.C_D.setdefault(W, el.c_bound(W))
        _BUILT[spec] = el.build_case(W, N, rows, k, bias=False, seed=2000 + 7 * W + N + rows + k)
    return _BUILT[spec]


def layer_tables(case, D, layers):
    """(the `layers` tables [num_users + N, D] f32, num_users): the column blocks of the case's tables."""
    num_users = case.U.shape[0]
    tables = [np.ascontiguousarray(np.concatenate([case.U[:, l * D:(l + 1) * D], case.I[:, l * D:(l + 1) * D]]))
              for l in range(layers)]
    return tables, num_users
