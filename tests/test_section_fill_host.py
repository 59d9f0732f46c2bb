"""`OT_DEFER_SECTIONS` and `ot_rays_fill_sections` at the C-ABI, as far as the host alone can tell: declared, bound, and
refusing what they must before anything is launched.  A scene handle needs a device (`ot_scene_create`), so the refusals that
come after the null checks -- section count, ray range, missing planes -- and what the mask does to a trace are marked `gpu`;
the planes themselves are in test_gpu_section_fill.py."""
import ctypes as C
import pathlib

import pytest

import optrace_amd as ot
from optrace_amd import _capi

import scenes

gpu = pytest.mark.gpu
HEADER = pathlib.Path(__file__).resolve().parent.parent / "include" / "optrace_amd.h"


def last_error() -> bytes:
    return _capi.load_library().ot_last_error()


def test_bit_and_entry_point_are_declared_and_bound():
    header = HEADER.read_text()
    assert "#define OT_DEFER_SECTIONS 4u" in header and _capi.OT_DEFER_SECTIONS == 4
    assert "int ot_rays_fill_sections(" in header and "ot_rays_fill_sections" in _capi.SIGNATURES
    assert _capi.SIGNATURES["ot_rays_fill_sections"] == _capi.SIGNATURES["ot_rays_fill_pol"]  # its sibling's arguments
    assert not _capi.OT_DEFER_SECTIONS & (_capi.OT_DEFER_INDEX | _capi.OT_DEFER_POL)
    assert _capi.load_library().ot_abi_version() == _capi.ABI_VERSION == 9


def test_null_arguments_are_refused_with_the_entry_points_name():
    lib = _capi.load_library()
    rays, rng = _capi.Rays(), (_capi.SourceRange * 1)()
    one = C.c_void_p(1)  # (never followed: every call below has a null in front of its first use)
    for args in ((None, None, None, 0, 0, None, 0, 0, None),
                 (None, one, rng, 1, 0, C.byref(rays), 0, 0, None),      # scene
                 (one, None, rng, 1, 0, C.byref(rays), 0, 0, None),      # sources
                 (one, one, None, 1, 0, C.byref(rays), 0, 0, None),      # ranges
                 (one, one, rng, 1, 0, None, 0, 0, None)):               # storage
        assert lib.ot_rays_fill_sections(*args) == -1  # OT_ERR_INVALID
        assert last_error() == b"ot_rays_fill_sections: null argument"
    for mask in (0, _capi.OT_DEFER_SECTIONS, 7, 8):
        assert lib.ot_scene_set_deferred_planes(None, mask) == -1 and b"ot_scene_set_deferred_planes: null scene" in last_error()


@pytest.fixture
def traced_scene():
    """(library, scene handle, source table, ranges, seed, ot_rays, tracer) of a small deferred trace."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=3)
        RT.trace(300)
    scene, tab, rng, seed, count = RT.rays._sections_stale
    assert count == 300
    return _capi.load_library(), scene.handle, tab, rng, seed, RT.rays._rays_struct(tail_only=True), RT


def variant(rays, **kw):
    r = _capi.Rays()
    C.memmove(C.byref(r), C.byref(rays), C.sizeof(r))
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@gpu
def test_refusals_each_with_its_message(traced_scene):
    lib, handle, tab, rng, seed, rays, RT = traced_scene

    def call(r, first=0, n=300):
        return lib.ot_rays_fill_sections(handle, tab.handle, rng, len(rng), seed, C.byref(r), first, n, None)

    for missing in ("p", "w", "s", "wl"):
        assert call(variant(rays, **{missing: None})) == -1
        assert last_error() == b"ot_rays_fill_sections: the ray storage needs p, w, s and wl"
    assert call(variant(rays, N=-1)) == -1 and b"ot_rays_fill_sections: the ray storage needs" in last_error()
    assert call(variant(rays, nt=rays.nt + 1)) == -1
    assert last_error() == b"ot_rays_fill_sections: ray storage has 18 sections, the scene needs 17"
    for first, n in ((-1, 1), (0, -1), (0, rays.N + 1), (rays.N, 1), (1, rays.N)):
        assert call(rays, first, n) == -1 and last_error() == b"ot_rays_fill_sections: range outside the storage"
    assert call(variant(rays, n=None, pol=None)) == 0  # neither the index plane nor the polarisation planes are used
    assert call(rays, rays.N, 0) == 0                  # an empty range at the end is a range


@gpu
def test_the_bit_round_trips_and_complete_storage_clears_it(traced_scene):
    lib, handle, tab, rng, seed, rays, RT = traced_scene
    raw = lambda: dict.__getitem__(RT.rays._dev, "p").view(3, RT.rays._nt, RT.rays._Np)[:, :, :300]

    def deferred_after(setter) -> bool:
        """Does a trace after `setter` leave the early sections of `p` alone?"""
        assert setter() == 0
        dict.__getitem__(RT.rays._dev, "p").fill_(-1.5)
        with ot.global_options.no_warnings():
            RT.trace(300)
        early, late = raw()[:, :-2], raw()[:, -2:]
        assert not bool((late == -1.5).any()), "the last two sections are always stored"
        assert bool((early == -1.5).all()) or not bool((early == -1.5).any()), "a section range is stored whole or not at all"
        return bool((early == -1.5).all())

    for mask in range(8):  # every combination of the three bits is a mask, and the sections follow their bit alone
        assert deferred_after(lambda: lib.ot_scene_set_deferred_planes(handle, mask)) == bool(mask & _capi.OT_DEFER_SECTIONS)
    assert lib.ot_scene_set_deferred_planes(handle, 8) == -1 and b"unknown bit in the mask" in last_error()
    assert deferred_after(lambda: lib.ot_scene_set_deferred_planes(handle, 7))
    assert not deferred_after(lambda: lib.ot_scene_set_index_store(handle, 1)), "on = 1 is complete storage: the whole mask goes"
    assert deferred_after(lambda: lib.ot_scene_set_deferred_planes(handle, _capi.OT_DEFER_SECTIONS))
    assert deferred_after(lambda: lib.ot_scene_set_index_store(handle, 0)), "on = 0 adds OT_DEFER_INDEX and leaves the other bits"
