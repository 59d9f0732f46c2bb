"""The `ot_spotdiag_*` entry points without a device: every refusal is answered from the arguments alone, before a device is looked
for; the workspace and the chunk count against their mirrors (tests/spot_diagram_cases.py)."""
import ctypes as C

import numpy as np

from optrace_amd import _capi

import spot_diagram_cases as sc

NAN = float("nan")
INVALID, UNSUPPORTED = -1, -3


def test_entry_points_check_their_arguments_before_anything_else():
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    dn = lambda *v: (C.c_double * len(v))(*v)
    ranges = lambda *v: (C.c_int64 * len(v))(*v)

    def rays(N=100, nt=3, p=a, w=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.wl = N, nt, p, w, wl
        return C.byref(r)

    def refused(code, text, status):
        assert status == code and text.encode() in lib.ot_last_error(), (status, lib.ot_last_error())

    #       0       1                     2  3  4  5  6  7            8  9           10
    head = [rays(), ranges(0, 10, 20, 5), 2, 1, a, 0, 3, dn(0, 0, 0), a, dn(0.5, 1), 2]
    extent = ("ot_spotdiag_extent", lambda *args: lib.ot_spotdiag_extent(*args, st), head + [a, a], (0, 1, 4, 7, 8, 9, 11, 12))
    #                                                                               11 12   13 14 15
    maps = ("ot_spotdiag_maps", lambda *args: lib.ot_spotdiag_maps(*args, st), head + [8, 0.5, a, a, a], (0, 1, 4, 7, 8, 9, 13, 14, 15))
    for name, call, ok, pointers in (extent, maps):
        for i in pointers:
            refused(INVALID, f"{name}: null argument", call(*[None if j == i else x for j, x in enumerate(ok)]))
        for R in (rays(p=None), rays(w=None)):
            refused(INVALID, f"{name}: null argument", call(R, *ok[1:]))
        for pair in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
            refused(INVALID, f"{name}: ray range", call(ok[0], ranges(0, 10, *pair), *ok[2:]))
        for k in (-1, 2, 100):
            refused(INVALID, f"{name}: section", call(*ok[:3], k, *ok[4:]))
        refused(INVALID, f"{name}: a field starts before key_first", call(*ok[:5], 1, *ok[6:]))
        for org in (dn(NAN, 0, 0), dn(0, np.inf, 0), dn(0, 0, -np.inf)):
            refused(INVALID, f"{name}: origin", call(*ok[:7], org, *ok[8:]))
        for zeta in (dn(NAN, 1), dn(0, -np.inf)):
            refused(INVALID, f"{name}: zeta not finite", call(*ok[:9], zeta, *ok[10:]))
        for K in (0, -1, 33):
            refused(UNSUPPORTED, f"{name}: n_fields outside 1 .. 64, n_bands outside 1 .. 32", call(*ok[:6], K, *ok[7:]))
        for F in (0, -1, 65):
            refused(UNSUPPORTED, f"{name}: n_fields outside 1 .. 64", call(*ok[:2], F, *ok[3:]))
        for Z in (0, -1, 66):
            refused(UNSUPPORTED, "n_planes outside 1 .. 65", call(*ok[:10], Z, *ok[11:]))
        # no ray in any field: nothing to do, whatever key_first is; the limits hold whatever the counts are
        assert call(ok[0], ranges(0, 0, 100, 0), *ok[2:5], 50, *ok[6:]) == 0
        refused(UNSUPPORTED, name, call(ok[0], ranges(0, 0, 100, 0), 2, 1, a, 0, 33, *ok[7:]))
    name, call, ok, _ = maps
    for n_px in (0, -1, 1025):
        refused(UNSUPPORTED, "ot_spotdiag_maps: n_px outside 1 .. 1024", call(*ok[:11], n_px, *ok[12:]))
    for size in (0.0, -1.0, NAN, np.inf, -np.inf):
        refused(INVALID, "ot_spotdiag_maps: size", call(*ok[:12], size, *ok[13:]))
    # F K Z n_px^2 above 2^28 cells: 2 x 3 x 2 x 1024^2 is below, 2 x 32 x 5 x 1024^2 above
    none = ranges(0, 0, 100, 0)
    assert call(ok[0], none, *ok[2:11], 1024, *ok[12:]) == 0
    refused(UNSUPPORTED, "ot_spotdiag_maps: more than 268435456 cells", call(ok[0], none, 2, 1, a, 0, 32, ok[7], a, dn(*range(5)), 5, 1024, *ok[12:]))
    assert call(ok[0], none, 2, 1, a, 0, 32, ok[7], a, dn(*range(4)), 4, 1024, *ok[12:]) == 0  # (2^28 exactly)


def test_workspace_and_chunks():
    lib = _capi.load_library()

    def ws(counts, K, Z):
        return lib.ot_spotdiag_workspace((C.c_int64 * (2 * len(counts)))(*[v for n in counts for v in (0, n)]), len(counts), K, Z)

    assert ws([1], 1, 1) == 16 and ws([256], 3, 3) == 18 and ws([257], 3, 4) == 2 * 2 * 18 and ws([0], 3, 1) == 18
    assert ws([10 ** 8], 1, 8) == 1024 * 16 and ws([10 ** 8], 3, 5) == 512 * 2 * 18 and ws([2 ** 28 + 1, 5], 32, 65) == 2 * 17 * 8 * 33 * 16
    for counts, K, Z in (([257, 0, 3000], 3, 3), ([70000], 4, 2), ([5000, 9000], 32, 65), ([1], 2, 1), ([300, 65], 5, 1)):
        assert ws(counts, K, Z) == sc.workspace(counts, K, Z)
    for counts, K, Z in (([-1], 3, 1), ([10], 0, 1), ([10], 33, 1), ([1] * 65, 1, 1), ([], 1, 1), ([10], 1, 0), ([10], 1, 66)):
        assert ws(counts, K, Z) == 0
    assert lib.ot_spotdiag_workspace(None, 1, 1, 1) == 0
    for K, Z, n_px in ((1, 1, 1), (3, 5, 64), (32, 65, 2), (32, 65, 16), (1, 1, 142), (1, 1, 143), (32, 65, 1024), (3, 3, 64), (5, 1, 5)):
        assert lib.ot_spotdiag_chunks(K, Z, n_px) == sc.chunks(K, Z, n_px)[0]
    assert lib.ot_spotdiag_chunks(3, 5, 64) == 4 and lib.ot_spotdiag_chunks(3, 3, 64) == 3
    for K, Z, n_px in ((0, 1, 1), (33, 1, 1), (1, 0, 1), (1, 66, 1), (1, 1, 0), (1, 1, 1025)):
        assert lib.ot_spotdiag_chunks(K, Z, n_px) == 0
