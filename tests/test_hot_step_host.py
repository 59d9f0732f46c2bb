"""The hot records of the step loop (csrc/ot_scene.hpp::HotStep) as the scene compiler writes them, on the host alone:
`ot_scene_records_host` compiles a scene description the way `ot_scene_create` does and hands back the hot records, the
surface records and the step records.  For every surface kind and the edges of the form decisions: the form code is the
one the device code's own comparisons would reach, every field of a hot record is bit for bit the SurfDev / StepDev
field it mirrors, and the table ends with one record of padding.  tests/test_gpu_hot_step.py holds the kernels that read
the records to the surface-record path."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi

import scenes

HEADER = pathlib.Path(__file__).resolve().parent.parent / "include" / "optrace_amd.h"
f8, i4 = "<f8", "<i4"
HOT = np.dtype([(n, i4) for n in "kind form surf n_next filter hurb hurb_slot _pad0".split()]
               + [(n, f8) for n in "px py pz r_eps2 z_max z_lo z_hi k1 inv_rho two_inv_rho k ri_eps2 nrho rho2 krho2 f fsign".split()]
               + [("_pad", f8, 3)])
SURF = np.dtype([(n, i4) for n in "kind ncoeff flat rot".split()]
                + [(n, f8) for n in ("px py pz r_eps2 ri_eps2 ox_lo ox_hi oy_lo oy_hi ix_lo ix_hi iy_lo iy_hi cna sna k k1 rho nrho "
                                     "rho2 k1rho2 krho2 inv_rho two_inv_rho z_min z_max z_lo z_hi z_beh zt1 zt2 edge_val r_edge ri "
                                     "hdx hdy cpa spa").split()]
                + [("coeff", f8, 12), ("dcoeff", f8, 12)]
                + [(n, f8) for n in "nx ny nz mx my sgn offs inv_h ku_t0 ku_h ku_inv_h ku_lo ku_hi".split()]
                + [("tab", "<u8"), ("nk", i4), ("deriv_unrot", i4), ("mask_off", "<i8"), ("mask_n", i4), ("mask_pad", i4),
                   ("mask_r", f8), ("mask_scale", f8)])
STEP = np.dtype([(n, i4) for n in "kind surf n_next filter hurb hurb_slot _pad0 _pad1".split()] + [("f", f8), ("fsign", f8)])
TABLES = {0: HOT, 1: SURF, 2: STEP}
FROM_SURF = "px py pz r_eps2 z_max z_lo z_hi k1 inv_rho two_inv_rho k ri_eps2 nrho rho2 krho2".split()
FROM_STEP = "kind surf n_next filter hurb hurb_slot f fsign".split()
STEP_LENS_FRONT, STEP_LENS_BACK, STEP_IDEAL, STEP_FILTER, STEP_APERTURE = range(5)


def records(desc, table: int, hot_steps: int = 1) -> np.ndarray:
    lib = _capi.load_library()
    n, size = C.c_int32(), C.c_int32()
    assert lib.ot_scene_records_host(C.byref(desc), table, hot_steps, None, 0, C.byref(n), C.byref(size)) == 0
    assert size.value == TABLES[table].itemsize
    buf = np.zeros(n.value, dtype=TABLES[table])
    assert lib.ot_scene_records_host(C.byref(desc), table, hot_steps, buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(size)) == 0
    assert n.value == buf.shape[0]
    return buf


class Desc:
    """A scene description around a list of (surface description, element kind, extra): lenses use the surface for both
    faces (the compiler looks at no geometry), a filter gets a constant spectrum, an ideal lens D = extra."""

    def __init__(self, items):
        self.surfaces = (_capi.Surface * len(items))(*[s for s, _, _ in items])
        self.elements = (_capi.Element * len(items))()
        self.media = (_capi.Medium * 2)()
        self.media[0].model, self.media[1].model = _capi.N_CONSTANT, _capi.N_CONSTANT
        self.media[0].c[0], self.media[1].c[0] = 1.0, 1.5
        self.filters = (_capi.Filter * 1)()
        self.filters[0].type, self.filters[0].val = _capi.T_CONSTANT, 0.5
        for i, (_, kind, extra) in enumerate(items):
            e = self.elements[i]
            e.kind, e.front = kind, i
            e.back = e.n_lens = e.n_after = e.filter = -1
            if kind == _capi.EL_LENS:
                e.back, e.n_lens, e.n_after = i, 1, 0
            elif kind == _capi.EL_IDEAL_LENS:
                e.n_after, e.D = 0, extra
            elif kind == _capi.EL_FILTER:
                e.filter = 0
        d = self.desc = _capi.SceneDesc()
        d.outline[:] = [-10., 10., -10., 10., -10., 100.]
        d.n_surfaces = d.n_elements = len(items)
        d.n_media, d.n_filters = 2, 1
        d.surfaces, d.elements, d.media, d.filters = self.surfaces, self.elements, self.media, self.filters


def expected_form(sf) -> int:
    """The decisions of find_hit, find_hit_conic and surf_normal for a surface record, restated."""
    if sf["kind"] == _capi.SURF_CIRCLE and sf["flat"]:
        return _capi.HOT_FLAT
    if sf["kind"] == _capi.SURF_RING and sf["flat"]:
        return _capi.HOT_RING
    if sf["kind"] != _capi.SURF_CONIC or sf["flat"]:
        return _capi.HOT_OTHER
    if sf["k"] != 0.0:
        return _capi.HOT_CONIC
    return _capi.HOT_SPHERE if abs(sf["inv_rho"]) <= 4096.0 else _capi.HOT_SPHERE_STABLE


def cases() -> list:
    """(name, surface description, element kind, extra, form)"""
    L, A = _capi.EL_LENS, _capi.EL_APERTURE
    with ot.global_options.no_warnings():
        zoo = scenes.surface_zoo(ot)
        forms = dict(circle=_capi.HOT_FLAT, ring=_capi.HOT_RING, rect=0, rect_rot=0, slit=0, slit_rot=0,
                     sphere_pos=_capi.HOT_SPHERE, sphere_neg=_capi.HOT_SPHERE, conic_m025=_capi.HOT_CONIC,
                     conic_m75=_capi.HOT_CONIC, conic_p3=_capi.HOT_CONIC, conic_parab=_capi.HOT_CONIC, asphere_a=0, asphere_b=0)
        out = [(name, sf._desc(), A if sf._desc().kind < _capi.SURF_CONIC else L, 0.0, forms[name]) for name, sf in zoo.items()]
        above = float(np.nextafter(4096.0, np.inf))
        out.append(("sphere_4096", ot.SphericalSurface(r=30., R=4096.)._desc(), L, 0.0, _capi.HOT_SPHERE))
        out.append(("sphere_m4096", ot.SphericalSurface(r=30., R=-4096.)._desc(), L, 0.0, _capi.HOT_SPHERE))
        # 1 / (1 / R) of the next double above 4096 is what the record holds and what the device compared: the rule on it
        inv = 1 / (1 / above)
        out.append(("sphere_above", ot.SphericalSurface(r=30., R=above)._desc(), L, 0.0,
                    _capi.HOT_SPHERE if abs(inv) <= 4096.0 else _capi.HOT_SPHERE_STABLE))
        out.append(("sphere_5000", ot.SphericalSurface(r=30., R=-5000.)._desc(), L, 0.0, _capi.HOT_SPHERE_STABLE))
        out.append(("k_m1", ot.ConicSurface(r=2., R=9., k=-1.)._desc(), L, 0.0, _capi.HOT_CONIC))
        out.append(("k_0_conic", ot.ConicSurface(r=2., R=9., k=0.)._desc(), L, 0.0, _capi.HOT_SPHERE))
        flat = ot.SphericalSurface(r=2., R=9.)._desc()
        flat.z_min = flat.z_max  # a conic record with a flat sag: find_hit_conic, but the normal of a plane
        out.append(("k_0_flat_sag", flat, L, 0.0, _capi.HOT_OTHER))
        ring = ot.RingSurface(r=4., ri=1.5)
        ring.move_to([0.25, -0.5, 3.])
        out.append(("ring_moved", ring._desc(), A, 0.0, _capi.HOT_RING))
        dec = ot.SphericalSurface(r=3., R=-12.)
        dec.move_to([0.7, -0.3, 5.])
        out.append(("decentred", dec._desc(), L, 0.0, _capi.HOT_SPHERE))
        rect = ot.RectangularSurface(dim=[3., 1.])
        rect.rotate(17.)
        out.append(("rect_17", rect._desc(), A, 0.0, _capi.HOT_OTHER))
        out.append(("tilted", ot.TiltedSurface(r=3., normal=[0.1, -0.2, 0.9])._desc(), L, 0.0, _capi.HOT_OTHER))
        out.append(("asphere", ot.AsphericSurface(r=3., R=20., k=0., coeff=[1e-4])._desc(), L, 0.0, _capi.HOT_OTHER))
        out.append(("ideal", ot.CircularSurface(r=3.)._desc(), _capi.EL_IDEAL_LENS, -12.5, _capi.HOT_FLAT))
        out.append(("ideal_rect", ot.RectangularSurface(dim=[3., 3.])._desc(), _capi.EL_IDEAL_LENS, 8.0, _capi.HOT_OTHER))
        out.append(("filter", ot.CircularSurface(r=2.)._desc(), _capi.EL_FILTER, 0.0, _capi.HOT_FLAT))
    return out


@pytest.fixture(scope="module")
def compiled():
    cs = cases()
    d = Desc([(s, kind, extra) for _, s, kind, extra, _ in cs])
    return cs, {hot: records(d.desc, 0, hot) for hot in (0, 1)}, records(d.desc, 1), records(d.desc, 2)


def test_entry_points_are_declared_and_bound():
    header = HEADER.read_text()
    for name in ("ot_scene_set_hot_steps", "ot_scene_read_hot_steps", "ot_scene_records_host"):
        assert f"int {name}(" in header and name in _capi.SIGNATURES
    lib = _capi.load_library()
    assert lib.ot_scene_set_hot_steps(None, 1) == -1 and b"ot_scene_set_hot_steps: null scene" in lib.ot_last_error()
    n = C.c_int32()
    assert lib.ot_scene_read_hot_steps(None, None, 0, C.byref(n)) == -1 and b"ot_scene_read_hot_steps: null argument" in lib.ot_last_error()
    assert lib.ot_scene_records_host(None, 0, 1, None, 0, C.byref(n), C.byref(n)) == -1
    d = Desc([(ot.CircularSurface(r=1.)._desc(), _capi.EL_APERTURE, 0.0)])
    assert lib.ot_scene_records_host(C.byref(d.desc), 3, 1, None, 0, C.byref(n), C.byref(n)) == -1
    buf = np.zeros(1, dtype=HOT)  # two records are needed
    assert lib.ot_scene_records_host(C.byref(d.desc), 0, 1, buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(n)) == -1
    assert b"buffer too small" in lib.ot_last_error()
    assert HOT.itemsize == 192 and SURF.itemsize == 664 and STEP.itemsize == 48


def test_steps_follow_the_elements(compiled):
    cs, hot, surfs, steps = compiled
    assert surfs.shape[0] == len(cs)
    kinds = []
    for _, _, kind, _, _ in cs:
        kinds += {_capi.EL_LENS: [STEP_LENS_FRONT, STEP_LENS_BACK], _capi.EL_IDEAL_LENS: [STEP_IDEAL],
                  _capi.EL_FILTER: [STEP_FILTER], _capi.EL_APERTURE: [STEP_APERTURE]}[kind]
    assert steps["kind"].tolist() == kinds
    ideal = steps[steps["kind"] == STEP_IDEAL]
    assert ideal["f"].tolist() == [1000 / -12.5, 1000 / 8.0] and ideal["fsign"].tolist() == [-1.0, 1.0]


def test_forms_are_the_device_codes_decisions(compiled):
    cs, hot, surfs, steps = compiled
    seen = set()
    for i, st in enumerate(steps):
        name, _, _, _, form = cs[st["surf"]]
        assert hot[1]["form"][i] == form == expected_form(surfs[st["surf"]]), name
        assert hot[0]["form"][i] == _capi.HOT_OTHER, name
        seen.add(form)
    assert seen == set(range(6))
    by_name = {name: surfs[j] for j, (name, *_) in enumerate(cs)}
    assert by_name["sphere_4096"]["inv_rho"] == 4096.0 and by_name["sphere_m4096"]["inv_rho"] == -4096.0
    assert by_name["sphere_above"]["inv_rho"] == 1 / (1 / np.nextafter(4096.0, np.inf))
    assert by_name["k_0_flat_sag"]["flat"] == 1 and by_name["k_0_conic"]["k"] == 0.0 and by_name["k_m1"]["k"] == -1.0
    assert by_name["decentred"]["px"] == 0.7 and by_name["decentred"]["py"] == -0.3


def test_fields_mirror_their_records_bit_for_bit(compiled):
    cs, hot, surfs, steps = compiled
    for on in (0, 1):
        h = hot[on]
        for i, st in enumerate(steps):
            sf, name = surfs[st["surf"]], cs[st["surf"]][0]
            for f in FROM_SURF:
                assert h[f][i].tobytes() == sf[f].tobytes(), (name, f)
            assert h["z_hi"][i].tobytes() == sf["z_beh"].tobytes(), name  # one field for both: z_max + N_EPS
            for f in FROM_STEP:
                assert h[f][i].tobytes() == st[f].tobytes(), (name, f)
            assert h["_pad0"][i] == 0 and not h["_pad"][i].any()
    a, b = hot[0].copy(), hot[1].copy()
    a["form"] = b["form"] = 0
    assert a.tobytes() == b.tobytes(), "the switch changes the forms alone"


def test_the_table_is_padded_by_one_record(compiled):
    cs, hot, surfs, steps = compiled
    for on in (0, 1):
        assert hot[on].shape[0] == steps.shape[0] + 1
        assert hot[on][-1:].tobytes() == bytes(HOT.itemsize)
    d = Desc([(ot.SphericalSurface(r=1., R=5.)._desc(), _capi.EL_APERTURE, 0.0)])  # one step
    one = records(d.desc, 0)
    assert one.shape[0] == 2 and one["form"][0] == _capi.HOT_SPHERE and one[1:].tobytes() == bytes(HOT.itemsize)
