"""Pins the oracle's detector stage (oracle/oracle.c::orc_detector_hits, the plain restatement of Raytracer._hit_detector,
raytracer.py:881-1051) to the reference for every detector kind at every placement: tests/golden/detectors.npz holds the
reference's ray sections of two scenes and, per (kind, placement, projection), its hits.  The fixture's generator keeps every
ray off the decision thresholds of the search, so no ray is excluded here.  CPU only."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi

import oracle_bridge as ob
import scenes
from detector_fixture import fixture, records, record_id
from helpers import assert_close, image_rel_l1


def test_fixture_holds_every_record_once():
    fx = fixture()
    want = [record_id(r) for r in records()]
    assert sorted(want) == sorted(str(k) for k in fx.g["rec/keys"]) and len(set(want)) == len(want)
    kinds = {r[1] for r in records("objective")}
    assert kinds == set(scenes.detector_kinds(ot)) == set(scenes.DETECTOR_CLOSED + scenes.DETECTOR_NUMERIC)
    for kind in kinds - {"tilted_ill"}:
        assert {r[2] for r in records("objective") if r[1] == kind} == set(scenes.DETECTOR_PLACEMENTS)
    assert fx.scene("objective")["p_list"].shape[1] != fx.scene("numeric")["p_list"].shape[1], "two section counts"
    assert any(fx.record(k)["ill"] > 0 for k in want)


def test_surfaces_no_detector_takes():
    """detector.py:39-41: data, function and aspheric surfaces are refused -- by the reference (the names the generator
    recorded) and here.  That is why no such detector has a record."""
    refused = {str(n) for n in fixture().g["refused"]}
    surfaces = scenes.detector_refused(ot)
    assert refused == set(surfaces)
    for name, surf in surfaces.items():
        with pytest.raises(RuntimeError):
            ot.Detector(surf, pos=[0, 0, 0])


@pytest.fixture(scope="module")
def host_rays():
    out = {}
    for name in scenes.DETECTOR_SCENES:
        sc = fixture().scene(name)
        out[name] = ob.HostRays.from_lists(sc["p_list"], sc["w_list"], sc["wl"])
    return out


@pytest.mark.parametrize("rec", records(), ids=record_id)
def test_oracle_detector_hits(rec, host_rays):
    name, kind, place, proj = rec
    fx = fixture()
    g, rays = fx.record(record_id(rec)), host_rays[name]
    with ot.global_options.no_warnings():
        surf = scenes.detector_kinds(ot)[kind]
    surf.move_to(g["pos"])
    ph, hw, ext, ill, st = ob.detector_hits(rays, 0, rays.N, surf._desc(), _capi.PROJECTIONS[proj])
    assert st == 0
    sel = hw > 0
    assert np.count_nonzero(sel) == g["w"].shape[0], "number of detector hits must be exact"
    assert np.array_equal(hw[sel], g["w"])
    assert np.array_equal(fx.scene(name)["wl"][sel], g["wl"])
    assert_close(ph[sel], g["ph"], rtol=1e-9, atol=1e-11, what="ph")
    assert ill == g["ill"]
    if np.any(sel):
        assert_close(ext, g["extent"], rtol=1e-9, atol=1e-11, what="extent")
    else:
        assert np.array_equal(g["extent"], np.repeat(g["pos"][:2], 2)), "without a hit: the detector's centre"
    # render with the reference's (fixed-up) extent.  Where the reference took the hits' own extent unchanged, the outermost
    # hits sit exactly on the image's border; the oracle's hits (equal to 1e-9 above, a sphere projection's atan / tan may differ
    # in the last bit) are then binned into their own extent, as the reference binned its own -- no hit falls off the border
    im = fx.image(record_id(rec))
    Ny, Nx = im["dense"].shape[:2]
    own = np.any(sel) and np.array_equal(im["extent"], g["extent"])
    img = ob.render(ph[sel, 0], ph[sel, 1], hw[sel], fx.scene(name)["wl"][sel], ext if own else im["extent"], Nx, Ny)
    assert abs(img[..., 3].sum() - im["power"]) <= 1e-12 * im["power"]
    if im["power"] > 0:
        assert np.all(image_rel_l1(img, im["dense"]) < 1e-4), image_rel_l1(img, im["dense"])
