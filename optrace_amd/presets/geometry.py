"""Geometry presets: an ideal camera and two schematic eye models (presets/geometry.py).

Numbers of the eye models from Schwiegerling, Field Guide to Visual and Ophthalmic Optics, SPIE 2004.  The reference adds
a display-only Volume (camera box, eye ball) to each group; volumes are not part of this package, so the groups hold the
optical elements only.
"""
from __future__ import annotations

import numpy as np

from ..base import check_above
from ..geometry import (Group, Lens, IdealLens, Aperture, Detector, ConicSurface, RingSurface, SphericalSurface,
                        RectangularSurface)
from ..refraction_index import RefractionIndex


def ideal_camera(cam_pos, z_g: float, b: float = 10, r: float = 6, r_det: float = 6) -> Group:
    """Ideally imaging camera: an ideal lens of radius `r` at `cam_pos` that images the plane z = `z_g` onto a square
    detector of half side `r_det` at the image distance `b` behind it (presets/geometry.py:15-48)."""
    check_above("b", b, 0)
    check_above("g = cam_pos[2] - z_g", cam_pos[2] - z_g, 0)
    g = cam_pos[2] - z_g
    D = (1 / b + 1 / g) * 1000   # imaging equation, mm -> dioptres
    objective = IdealLens(pos=cam_pos, r=r, D=D, long_desc="Camera Objective", desc="Obj")
    sensor = Detector(RectangularSurface([2 * r_det, 2 * r_det]), pos=np.array(cam_pos) + [0, 0, b],
                      long_desc="Camera Sensor", desc="Sensor")
    return Group([objective, sensor], long_desc="Ideal Camera", desc="Camera")


def arizona_eye(adaptation: float = 0., pupil: float = 5.7, r_det: float = 8, pos: list = None) -> Group:
    """Arizona eye model (Schwiegerling, Field Guide to Visual and Ophthalmic Optics, SPIE 2004), as in
    presets/geometry.py:54-108: cornea, pupil, lens with accommodation-dependent conics, spherical retina."""
    origin = np.zeros(3) if pos is None else np.array(pos, dtype=np.float64)
    A = adaptation
    gap_aqueous, gap_lens, cornea_thickness = 2.97 - 0.04 * A, 3.767 + 0.04 * A, 0.55

    def at(z: float) -> np.ndarray:
        return origin + [0, 0, z]

    # media: name -> (n at the centre line, Abbe number)
    table = dict(Cornea=(1.377, 57.1), Aqueous=(1.337, 61.3), Vitreous=(1.336, 61.1),
                 Lens=(1.42 + 0.00256 * A - 0.00022 * A ** 2, 51.9))
    n = {name: RefractionIndex("Abbe", n=nc, V=V, desc=f"n_{name}") for name, (nc, V) in table.items()}

    eye = Group(desc="Eye", long_desc="Arizona Eye Model")
    cornea = Lens(ConicSurface(r=5.45, R=7.8, k=-0.25, long_desc="Cornea Anterior"),
                  ConicSurface(r=5.45, R=6.5, k=-0.25, long_desc="Cornea Posterior"),
                  d1=0, d2=cornea_thickness, pos=at(0), n=n["Cornea"], n2=n["Aqueous"], desc="Cornea")
    eye.add(cornea)
    eye.add(Aperture(RingSurface(r=5.45, ri=pupil / 2, desc="Pupil"),
                     pos=at(cornea.back.pos[2] + gap_aqueous - 1e-9), desc="Pupil"))
    eye.add(Lens(ConicSurface(r=5.1, R=12 - 0.4 * A, k=-7.518749 + 1.285720 * A, long_desc="Lens Anterior"),
                 ConicSurface(r=5.1, R=-5.224557 + 0.2 * A, k=-1.353971 - 0.431762 * A, long_desc="Lens Posterior"),
                 d1=0, d2=gap_lens, pos=at(gap_aqueous + cornea_thickness), n=n["Lens"], n2=n["Vitreous"],
                 desc="Lens"))
    eye.add(Detector(SphericalSurface(r=r_det, R=-13.4, desc="Retina"), pos=at(24), desc="Retina"))
    return eye


def legrand_eye(pupil: float = 5.7, r_det: float = 8., pos: list = None) -> Group:
    """LeGrand full theoretical eye (same source; presets/geometry.py:122-186): a paraxial schematic eye relaxed to
    infinity, spherical surfaces and media without dispersion.  Good for first-order properties only."""
    origin = np.zeros(3) if pos is None else np.array(pos, dtype=np.float64)

    def at(z: float) -> np.ndarray:
        return origin + [0, 0, z]

    table = dict(Cornea=1.3771, Aqueous=1.3374, Lens=1.4200, Vitreous=1.3360)
    n = {name: RefractionIndex("Constant", n=value, desc=f"n_{name}") for name, value in table.items()}

    eye = Group(desc="Eye", long_desc="LeGrand Full Theoretical Eye")
    eye.add(Lens(SphericalSurface(r=5.5, R=7.8, long_desc="Cornea Anterior"),
                 SphericalSurface(r=5.5, R=6.5, long_desc="Cornea Posterior"),
                 d1=0.25, d2=0.30, pos=at(0.25), n=n["Cornea"], n2=n["Aqueous"], desc="Cornea"))
    # the pupil sits on the anterior lens vertex, z = 3.6 mm
    eye.add(Aperture(RingSurface(r=5.5, ri=pupil / 2, desc="Pupil"), pos=at(3.6), desc="Pupil"))
    eye.add(Lens(SphericalSurface(r=4.8, R=10.2, long_desc="Lens Anterior"),
                 SphericalSurface(r=4.8, R=-6, long_desc="Lens Posterior"),
                 d1=1.5, d2=2.5, pos=at(5.10), n=n["Lens"], n2=n["Vitreous"], desc="Lens"))
    eye.add(Detector(SphericalSurface(r=r_det, R=-13.4, desc="Retina"), pos=at(24.197), desc="Retina"))
    return eye


eye_models: list = [legrand_eye, arizona_eye]

geometries: list = [ideal_camera, *eye_models]
