"""Error and argument cases of the paraxial analysis: name -> callable(); the fixture (tests/golden/tma.npz, "raises/...")
holds the class name of what the reference raises for each, or "none".  Run with either package, like host_cases.py."""
from __future__ import annotations

import numpy as np


def cases(ot) -> dict:
    n = ot.RefractionIndex("Constant", n=1.5)
    water = ot.RefractionIndex("Constant", n=1.33)

    def lens(z=0., x=0., y=0., front=None, back=None):
        return ot.Lens(front or ot.SphericalSurface(r=3, R=20), back or ot.SphericalSurface(r=3, R=-20), n=n,
                       pos=[x, y, z], de=0.2)

    def saddle():
        return ot.FunctionSurface2D(r=3, func=lambda x, y: (x ** 2 - y ** 2) / 50)  # no parax_roc

    xy = np.linspace(-3, 3, 60)
    X, Y = np.meshgrid(xy, xy)
    thick = lambda z: ot.Lens(ot.CircularSurface(r=3), ot.CircularSurface(r=3), n=n, pos=[0, 0, z], d=4.)  # noqa: E731
    return {
        "ok": lambda: ot.TMA([lens(), lens(10.)], wl=500., n0=water),
        "ok_int_wl": lambda: ot.TMA([lens()], wl=500),
        "off_axis_x": lambda: ot.TMA([lens(), lens(10., x=0.01)]),
        "off_axis_y": lambda: ot.TMA([lens(), lens(10.), lens(20., y=-0.5)]),
        "off_axis_within_rounding": lambda: ot.TMA([lens(), lens(10., x=1e-10)]),
        "no_parax_roc_front": lambda: ot.TMA([lens(front=saddle())]),
        "no_parax_roc_back": lambda: ot.TMA([lens(back=ot.DataSurface2D(r=3, data=X * Y / 40))]),
        "no_parax_roc_lens_tma": lambda: lens(front=saddle()).tma(),
        "overlap": lambda: ot.TMA([thick(0.), thick(3.)]),
        "overlap_group": lambda: ot.Group([thick(0.), thick(3.)]).tma(),
        "touching": lambda: ot.TMA([thick(0.), thick(4.)]),
        "wl_below": lambda: ot.TMA([lens()], wl=379.9),
        "wl_above": lambda: ot.TMA([lens()], wl=780.1),
        "wl_lens_tma": lambda: lens().tma(wl=100.),
        "wl_group_tma": lambda: ot.Group([lens()]).tma(wl=1000.),
        "wl_str": lambda: ot.TMA([lens()], wl="555"),
        "wl_none": lambda: ot.TMA([lens()], wl=None),
        "wl_array": lambda: ot.TMA([lens()], wl=np.array([555.])),
        "lenses_tuple": lambda: ot.TMA((lens(),)),
        "lenses_lens": lambda: ot.TMA(lens()),
        "lenses_none": lambda: ot.TMA(None),
        "n0_float": lambda: ot.TMA([lens()], n0=1.33),
        "n0_spectrum": lambda: ot.TMA([lens()], n0=ot.TransmissionSpectrum("Constant", val=1.)),
        "n0_lens_tma": lambda: lens().tma(n0="water"),
        "desc_type": lambda: ot.TMA([lens()], desc=5),
        "unknown_kwarg": lambda: ot.TMA([lens()], colour="red"),
        "locked": lambda: setattr(ot.TMA([lens()]), "wl", 600.),
        "locked_new_name": lambda: setattr(ot.TMA([lens()]), "focus", 1.),
        "object_inside": lambda: ot.TMA([lens(), lens(10.)]).image_position(5.),
        "object_inside_magnification": lambda: ot.TMA([lens(), lens(10.)]).image_magnification(5.),
        "image_inside": lambda: ot.TMA([lens(), lens(10.)]).object_position(5.),
        "image_inside_magnification": lambda: ot.TMA([lens(), lens(10.)]).object_magnification(5.),
        "object_on_vertex": lambda: ot.TMA([lens()]).image_position(float(lens().front.pos[2])),
        "object_inside_ideal": lambda: ot.TMA([ot.IdealLens(r=3, D=10., pos=[0, 0, 2])]).image_position(2.),
        "matrix_inside": lambda: ot.TMA([lens(), lens(10.)]).matrix_at(5., 6.),
        "pupil_inside": lambda: ot.TMA([lens(), lens(10.)]).pupil_position(5.),
    }


def outcome(case) -> str:
    try:
        case()
    except Exception as err:  # noqa: BLE001 -- the class is what is recorded
        return type(err).__name__
    return "none"
