"""Shared by tests/test_mf_wide_host.py and tests/test_gpu_mf_wide.py: the certified score ladders of the wide
embedding widths (256 / 512 / 1024), built once per session."""
import eval_ladders as el

WIDE = (256, 512, 1024)
for _D in WIDE:
    el.C_D.setdefault(_D, el.c_bound(_D))     # the existing bound formula: 1.56e-5, 3.09e-5, 6.14e-5

# (D, N, rows, k, bias).  33 items: a single ragged tile; 4,100: two slices; 16,411: eight slices and the library's
# prescan rule; 5 / 130 / 300 rows: a partial wave, one workgroup plus two rows, three workgroups with a ragged last.
# (1024, 16411, 130, 16, True) does not certify — the bias ladder's gaps fall below the bound — and is left out.
LADDER_SPECS = [
    (256, 33, 300, 1, False), (256, 4100, 300, 10, True), (256, 16411, 300, 16, False),
    (512, 4100, 5, 10, False), (512, 16411, 300, 10, True), (512, 33, 130, 16, True), (512, 4100, 300, 16, True),
    (1024, 4100, 300, 10, False), (1024, 16411, 130, 16, False), (1024, 16411, 130, 10, True),
    (1024, 33, 5, 1, False), (1024, 4100, 130, 1, True),
]
_BUILT = {}


def spec_id(s):
    return "D{}-N{}-n{}-k{}-{}".format(*s[:4], "bias" if s[4] else "nobias")


def ladder_case(spec):
    """build_case() certifies (asserts) the case it returns."""
    if spec not in _BUILT:
        D, N, n, k, bias = spec
        _BUILT[spec] = el.build_case(D, N, n, k, bias=bias, seed=1000 + 7 * D + N + n + k + bias)
    return _BUILT[spec]
