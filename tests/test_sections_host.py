"""The section table (`optrace_amd.scene.SectionTable`) without a device: ray section i of a trace against the scene's elements,
the one walk behind `Group.tracing_surfaces`, the names in a trace's warnings, the labels of `Raytracer.footprints`, the ideal-lens
warning of the wavefront and PSF analyses, and the z ranges of `focus_search` and of render-only chunks."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.scene import SectionTable

import host_cases
import scenes

OUTLINE = [-5, 5, -5, 5, -10, 40]
N15 = ot.RefractionIndex("Constant", n=1.5)


def parent_surface_names(RT) -> list:
    """`Raytracer._surface_names` as it was before the section table, kept to show that the names of a scene without an ideal lens
    did not change: by kind, `has_back()` (true for an ideal lens), then sorted by each surface's own z."""
    labelled = []
    for kind, group in (("Lens", RT.lenses), ("Aperture", RT.apertures), ("Filter", RT.filters)):
        for k, el in enumerate(group):
            tag = f"{kind} {el.abbr}{k}"
            if el.has_back():
                labelled += [(el.front.pos[2], f"front surface of {tag}"), (el.back.pos[2], f"back surface of {tag}")]
            else:
                labelled.append((el.pos[2], f"surface of {tag}"))
    labelled.sort(key=lambda item: item[0])
    return ["RaySource"] + [name for _, name in labelled] + ["Outline"]


def tracer(*elements):
    RT = ot.Raytracer(outline=OUTLINE)
    RT.add(ot.RaySource(ot.CircularSurface(r=1), pos=[0, 0, -5]))
    for el in elements:
        RT.add(el)
    return RT


def real_lens(z):
    return ot.Lens(ot.SphericalSurface(r=2, R=10), ot.SphericalSurface(r=2, R=-10), d=1, pos=[0, 0, z], n=N15)


def aperture(z):
    return ot.Aperture(ot.RingSurface(r=3, ri=1), pos=[0, 0, z])


def filter_(z):
    return ot.Filter(ot.CircularSurface(r=3), pos=[0, 0, z], spectrum=ot.TransmissionSpectrum("Constant", val=0.5))


def scene_a():
    """Two real lenses, an aperture between them, a filter behind; the lens at the larger z is added first: it is L0."""
    return tracer(real_lens(20), filter_(30), real_lens(5), aperture(12))


def scene_b():
    """Single-surface elements only, out of z order as well."""
    return tracer(filter_(15), aperture(25), aperture(5), filter_(10))


def scene_ideal():
    return tracer(real_lens(5), ot.IdealLens(r=3, D=20, pos=[0, 0, 10]), aperture(15), filter_(20))


# ---- 1. identity and count ------------------------------------------------------------------------------------------------------
# (scenes.objective and scenes.detector_objective are not here: they trace on the device while they are built)
BUILDERS = ["c1_single_lens", "double_gauss", "mixed_geometry", "arizona_eye_scene", "hurb_slit_lens", "hurb_ring_ideal",
            "asphere_scene", "prism_scene", "freeform_scene", "freeform_hurb_scene", "masked_scene", "masked_flat_scene",
            "double_gauss_aspheric", "detector_numeric", "c3_arizona_eye_rgb", "c4_image_render",
            "random_scene/1", "random_scene/2", "random_scene/3"]


def check_against_tracing_surfaces(RT):
    table = SectionTable(RT)
    surfaces = RT.tracing_surfaces
    assert table.nt == len(surfaces) + 2 and len(table.surfaces) == len(surfaces)
    assert all(mine is theirs for mine, theirs in zip(table.surfaces, surfaces))
    assert len(table.names()) == table.nt and len(table.labels("first")) == table.nt
    for row in table.rows:
        assert getattr(RT, {"Lens": "lenses", "Aperture": "apertures", "Filter": "filters"}[row.kind])[row.index] is row.element
        assert row.surface is (row.element.back if row.side == "back" else row.element.front)
        assert row.abbr == row.element.abbr and row.ideal == isinstance(row.element, ot.IdealLens)
    return table


@pytest.mark.parametrize("name", BUILDERS)
def test_table_is_tracing_surfaces_for_the_test_scenes(name):
    with ot.global_options.no_warnings():
        if name.startswith("random_scene/"):
            RT = scenes.random_scene(ot, int(name.split("/")[1]))
        else:
            RT = getattr(scenes, name)(ot)
    check_against_tracing_surfaces(RT)


def test_table_is_tracing_surfaces_for_the_host_case_elements():
    lenses, singles = host_cases.elements(ot)
    with ot.global_options.no_warnings():
        els = [make() for make in lenses.values()] + [make() for make in singles.values()]
        RT = ot.Raytracer(outline=[-10, 10, -10, 10, -10, 40])
        for el in els:
            RT.add(el)
    table = check_against_tracing_surfaces(RT)
    assert table.nt == 5 * 2 + 3 + 2  # five lenses, aperture, filter, ideal lens; the detector and the source have no section
    # a Group without sources of its own, with the sources handed in
    G = ot.Group([real_lens(5), aperture(12)])
    table = SectionTable(G, sources=RT.ray_sources)
    assert table.nt == 5 and all(a is b for a, b in zip(table.surfaces, G.tracing_surfaces)) and table.sources == RT.ray_sources


# ---- 2. literal strings -----------------------------------------------------------------------------------------------------------
def test_names_and_labels_two_lenses_aperture_filter():
    RT = scene_a()
    table = check_against_tracing_surfaces(RT)
    names = ["RaySource", "front surface of Lens L1", "back surface of Lens L1", "surface of Aperture AP0",
             "front surface of Lens L0", "back surface of Lens L0", "surface of Filter F0", "Outline"]
    assert table.names() == names and parent_surface_names(RT) == names
    assert table.labels("RS0") == ["RS0", "L1 front", "L1 back", "AP0", "L0 front", "L0 back", "F0", "end"]
    assert table.labels("sources")[0] == "sources"
    assert [row.index for row in table.rows] == [1, 1, 0, 0, 0, 0] and [row.side for row in table.rows] == ["front", "back", "", "front", "back", ""]
    assert not any(table.ideal_before(k) for k in range(table.nt))


def test_names_and_labels_single_surface_elements():
    RT = scene_b()
    table = check_against_tracing_surfaces(RT)
    names = ["RaySource", "surface of Aperture AP1", "surface of Filter F1", "surface of Filter F0", "surface of Aperture AP0", "Outline"]
    assert table.names() == names and parent_surface_names(RT) == names
    assert table.labels("sources") == ["sources", "AP1", "F1", "F0", "AP0", "end"]


def test_names_and_labels_empty_geometry():
    table = check_against_tracing_surfaces(tracer())
    assert table.nt == 2 and table.names() == ["RaySource", "Outline"] and table.labels("RS0") == ["RS0", "end"]
    assert not table.ideal_before(0)


def test_names_follow_the_tracing_order_where_surfaces_interleave_in_z():
    """A ring aperture around the bulge of a lens's back: its z (7.2) lies before the back's vertex (7.5), the geometry checks pass
    (on the ring the back lies below 7.2), and the trace meets the back first.  The parent sorted the names by each surface's z."""
    RT = tracer(ot.Lens(ot.CircularSurface(r=2), ot.SphericalSurface(r=2, R=-3), d1=0.5, d2=2.5, pos=[0, 0, 5], n=N15),
                ot.Aperture(ot.RingSurface(r=2, ri=1.5), pos=[0, 0, 7.2]))
    RT._geometry_checks()
    assert not RT.geometry_error
    table = check_against_tracing_surfaces(RT)
    assert [float(s.pos[2]) for s in table.surfaces] == [4.5, 7.5, 7.2]
    assert table.names() == ["RaySource", "front surface of Lens L0", "back surface of Lens L0", "surface of Aperture AP0", "Outline"]
    assert parent_surface_names(RT)[2:4] == ["surface of Aperture AP0", "back surface of Lens L0"]


# ---- 3. ideal lens ----------------------------------------------------------------------------------------------------------------
def test_ideal_lens_is_one_section():
    RT = scene_ideal()
    table = check_against_tracing_surfaces(RT)
    assert table.nt == 7
    assert table.names() == ["RaySource", "front surface of Lens L0", "back surface of Lens L0", "surface of Lens L1",
                             "surface of Aperture AP0", "surface of Filter F0", "Outline"]
    assert table.labels("RS0") == ["RS0", "L0 front", "L0 back", "L1", "AP0", "F0", "end"]
    assert [table.ideal_before(k) for k in range(6)] == [False, False, False, True, True, True]
    assert len(parent_surface_names(RT)) == 8  # (what the parent gave: one name more than there are sections)


def test_warning_behind_an_ideal_lens_names_its_own_surface():
    """A counter at section 4 of lens, ideal lens, aperture, filter is a count at the aperture.  The parent reports
    `surface 4 (back surface of Lens L1)` for the same counter: it gave the ideal lens two names."""
    RT = scene_ideal()
    RT._msgs = np.zeros((len(RT.INFOS), 7), dtype=int)
    RT._msgs[RT.INFOS.OUTLINE_INTERSECTION, 4] = 1
    with pytest.warns(ot.OptraceWarning) as caught:
        RT._show_messages(1000)
    assert len(caught) == 1
    text = str(caught[0].message)
    assert "surface 4 (surface of Aperture AP0)" in text and text.startswith("1 rays (0.1% of all rays) hitting outline after")
    assert parent_surface_names(RT)[4] == "back surface of Lens L1"


# ---- 4. gap and last z --------------------------------------------------------------------------------------------------------------
def test_gap_and_last_z():
    RT = scene_a()
    table = SectionTable(RT)
    L0, L1 = RT.lenses
    eps, z_end = RT.N_EPS, OUTLINE[5]
    # the spherical fronts (R = 10, r = 2) rise from their vertex by 10 - sqrt(96); the backs fall to theirs by as much
    sag = 10 - np.sqrt(96.0)
    assert L1.front.z_min == pytest.approx(4.5) and L1.front.z_max == pytest.approx(4.5 + sag)
    assert L1.back.z_max == pytest.approx(5.5) and L0.front.z_min == pytest.approx(19.5)
    # before the first surface: from the source's end (a flat disc at z = -5) to the first front's vertex
    assert table.gap(0.0, z_end, eps) == [-5 + eps, float(L1.front.z_min)]
    # between the first lens and the aperture (flat, z = 12)
    assert table.gap(8.0, z_end, eps) == [float(L1.back.z_max), 12.0]
    # behind the filter (flat, z = 30): to the outline's far face
    assert table.gap(35.0, z_end, eps) == [30.0, 40 - eps]
    assert table.z_last() == 30.0
    # a source that ends behind every surface is the last z
    RT.add(ot.RaySource(ot.CircularSurface(r=1), pos=[0, 0, 33]))
    assert SectionTable(RT).z_last() == 33.0 and SectionTable(RT).gap(35.0, z_end, eps) == [30.0, 40 - eps]


def test_origin_axes_and_radii():
    RT = scene_a()
    RT.add(ot.RaySource(ot.Point(), pos=[1, -2, -6]))
    table = SectionTable(RT)
    assert list(table.origin(0)) == [0, 0, -5] and list(table.origin(0, 0)) == [0, 0, -5] and list(table.origin(0, 1)) == [1, -2, -6]
    assert all(table.origin(k, 1) is table.surfaces[k - 1].pos or np.array_equal(table.origin(k, 1), table.surfaces[k - 1].pos)
               for k in range(1, table.nt - 1))
    axis, radii = table.axes_and_radii(1)
    assert [list(map(float, a)) for a in axis] == [[1, -2]] + [[0, 0]] * 7
    assert np.isnan(radii[0]) and np.isnan(radii[-1]) and radii[1:-1] == [2, 2, 3, 2, 2, 3]
