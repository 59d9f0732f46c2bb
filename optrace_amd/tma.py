"""Paraxial ray-transfer-matrix analysis of a lens system (optrace/tracer/transfer_matrix_analysis.py:17-368).

Host-only by design: a handful of 2 x 2 matrices per lens, evaluated once per call, nothing per ray.  A `TMA` is a locked
snapshot of the lenses as they were when it was made; it is no element of a scene and untracked (base.mutation_epoch),
so making one between two traces leaves `Raytracer.trace`'s unchanged-scene shortcut in place.

The vectors are (height, angle) columns, a system matrix maps the front vertex plane to the back vertex plane, and
`_steps` keeps every factor of it together with the distance from the front vertex at which that factor ends: the pupil
methods cut the chain there into the group in front of the stop and the group behind it.

Refraction indices are evaluated on the host, at the one wavelength of the analysis in float64
(`refraction_index.index_at`): `RefractionIndex.__call__` is a device call on wavelengths stored as float32, which a
paraxial analysis must not need and whose rounding of the wavelength the reference's analysis does not have.
"""
from __future__ import annotations

import numpy as np

from .base import BaseClass, check_type, check_not_below, check_not_above
from .options import global_options
from .refraction_index import RefractionIndex, index_at

_NAN2 = (float("nan"), float("nan"))


def _shift(dz: float) -> np.ndarray:
    """Free propagation over dz."""
    return np.array([[1, dz], [0, 1]])


def _interface(n_in: float, n_out: float, roc: float) -> np.ndarray:
    """Refraction from n_in into n_out at a surface with paraxial radius of curvature roc."""
    return np.array([[1, 0], [-(n_out - n_in) / roc / n_out, n_in / n_out]])


def _chain(factors: list) -> np.ndarray:
    """Matrix of the factors applied first to last."""
    total = np.eye(2)
    for m in reversed(factors):
        total = total @ m
    return total


def _between(abcd: np.ndarray, g: float, b: float) -> np.ndarray:
    """`abcd` with a path g in front of it and a path b behind it."""
    return _shift(b) @ abcd @ _shift(g)


def _conjugate(abcd: np.ndarray, dist: float, backwards: bool = False) -> float:
    """Image distance behind a system for an object `dist` in front of it; backwards: object distance in front for an
    image `dist` behind (the inverse system, looked at from behind).  An infinite distance gives the focal plane,
    NaN stands for "at infinity / undefined"."""
    if backwards:
        abcd, dist = np.linalg.inv(abcd), -dist
    A, B, C, D = abcd.ravel()
    if np.isfinite(dist):
        den = D + C * dist
        other = -(B + dist * A) / den if den else np.nan
    else:
        other = -A / C if C else np.nan
    return -other if backwards else other


class TMA(BaseClass):
    """Cardinal points, focal lengths, powers and imaging relations of centred lenses at one wavelength."""

    _tracked = False  # a result, not part of any scene

    def __init__(self, lenses: list, wl: float = 555., n0: RefractionIndex = None, **kwargs) -> None:
        check_type("lenses", lenses, list)
        check_type("n0", n0, (RefractionIndex, type(None)))
        check_type("wl", wl, (float, int))
        check_not_below("wl", wl, global_options.wavelength_range[0])
        check_not_above("wl", wl, global_options.wavelength_range[1])

        self.wl = wl
        order = sorted(lenses, key=lambda L: L.front.pos[2])
        self.vertex_points = (float(order[0].front.pos[2]), float(order[-1].back.pos[2])) if order else _NAN2
        self.n1 = index_at(n0, wl) if n0 is not None else 1.0
        self.n2 = index_at(order[-1].n2, wl) if order and order[-1].n2 is not None else self.n1
        v1, v2 = self._v1, self._v2 = self.vertex_points

        self._steps = self._factors(order)  # [(end of the factor behind the front vertex, matrix), ...]
        self.abcd = _chain([m for _, m in self._steps])
        A, B, C, D = (float(v) for v in self.abcd.ravel())
        n1, n2 = self.n1, self.n2
        focal = C != 0  # an afocal system (and no system at all) has no cardinal points

        self.principal_points = (v1 - (n1 - n2 * D) / (n2 * C), v2 + (1 - A) / C) if focal else _NAN2
        self.nodal_points = (v1 - (1 - D) / C, v2 + (n1 - n2 * A) / (n2 * C)) if focal else _NAN2
        p1, p2 = self.principal_points
        self.focal_points = (p1 + n1 / n2 / C, p2 - 1 / C) if focal else _NAN2
        F1, F2 = self.focal_points
        self.focal_lengths = (F1 - p1, F2 - p2) if focal else _NAN2
        f1, f2 = self.focal_lengths
        self.ffl = F1 - v1 if focal else _NAN2[0]
        self.bfl = F2 - v2 if focal else _NAN2[0]
        self.d = v2 - v1
        self.efl = f2
        self.efl_n = f2 / n2
        self.focal_lengths_n = (f1 / n1, f2 / n2)
        self.powers = (1000 / f1, 1000 / f2)
        self.powers_n = (1000 * n1 / f1, 1000 * n2 / f2)

        # the optical centre divides the thickness as 1 : (share - 1); D = 1 puts it on the front vertex
        share = 1 - A + B * C / (D - 1) if D - 1 else float("inf")
        ok = focal and share and not np.isnan(share)
        self.optical_center = v1 + self.d / share if ok else float("nan")

        BaseClass.__init__(self, **kwargs)
        self.lock()

    def _factors(self, order: list) -> list:
        """The system as (distance of the factor's end from the front vertex, matrix) in the order light meets them."""
        steps, z = [], 0
        for i, L in enumerate(order):
            nxt = order[i + 1] if i + 1 < len(order) else None
            if nxt is not None and not (np.isclose(L.pos[0], nxt.pos[0]) and np.isclose(L.pos[1], nxt.pos[1])):
                raise RuntimeError("Lenses don't share one axis.")
            before = order[i - 1].n2 if i else None
            n_in = index_at(before, self.wl) if before is not None else self.n1
            n_out = index_at(L.n2, self.wl) if L.n2 is not None else self.n1
            if L.is_ideal:
                steps.append((z, np.array([[1, 0], [-L.D / 1000, n_in / n_out]])))
            else:
                if L.front.parax_roc is None or L.back.parax_roc is None:
                    raise RuntimeError("Lens without rotational symmetry in transfer matrix analysis.")
                n = index_at(L.n, self.wl)
                steps.append((z, _interface(n_in, n, L.front.parax_roc)))
                z = z + L.d
                steps.append((z, _shift(L.d)))
                steps.append((z, _interface(n, n_out, L.back.parax_roc)))
            if nxt is not None:
                gap = nxt.front.pos[2] - L.back.pos[2]
                z = z + gap
                steps.append((z, _shift(gap)))
                if gap < 0:
                    raise RuntimeError("Negative distance between lenses. Are there object collisions?")
        return steps

    # ---- imaging -------------------------------------------------------------------------------------------
    def _outside(self, z: float, what: str) -> None:
        if self._v1 < z < self._v2:
            raise ValueError(f"{what} inside lens with z-extent at optical axis of {self.vertex_points}")

    def image_position(self, z_g) -> float:
        """z of the image of an object plane at z_g (+-inf: the back focal plane)."""
        self._outside(z_g, "Object")
        return float(_conjugate(self.abcd, self._v1 - z_g) + self._v2)

    def object_position(self, z_b) -> float:
        """z of the object plane that is imaged to z_b (+-inf: the front focal plane)."""
        self._outside(z_b, "Image")
        return float(self._v1 - _conjugate(self.abcd, z_b - self._v2, backwards=True))

    def matrix_at(self, z_g: float, z_b: float) -> np.ndarray:
        """System matrix from the plane z_g to the plane z_b."""
        return _between(self.abcd, self._v1 - z_g, z_b - self._v2)

    def image_magnification(self, z_g) -> float:
        """Image size over object size for an object plane at z_g."""
        with np.errstate(invalid="ignore"):
            return float(self.matrix_at(z_g, self.image_position(z_g))[0, 0])

    def object_magnification(self, z_b) -> float:
        """Image size over object size for an image plane at z_b."""
        with np.errstate(invalid="ignore"):
            return float(self.matrix_at(self.object_position(z_b), z_b)[0, 0])

    # ---- pupils --------------------------------------------------------------------------------------------
    def _pupils(self, z_s: float) -> tuple:
        """(entrance pupil z, exit pupil z, entrance magnification, exit magnification) of a stop at z_s: the stop imaged
        backwards through everything in front of it and forwards through everything behind it."""
        ends = [z for z, _ in self._steps]
        mats = [m for _, m in self._steps]
        cut = 0  # number of factors that end in front of the stop
        while cut < len(ends) and ends[cut] + self._v1 < z_s:
            cut += 1

        z_in, m_in = z_s, 1  # nothing in front: the stop is its own entrance pupil
        if cut:
            back = np.linalg.inv(_chain(mats[:cut]))  # (used from behind)
            dist = ends[cut - 1] + self._v1 - z_s  # from the front group's last vertex to the stop, negative
            z_in = self._v1 + _conjugate(back, dist)
            m_in = _between(back, dist, z_in - self._v1)[0, 0]

        z_out, m_out = z_s, 1  # nothing behind: the stop is its own exit pupil
        if cut < len(mats):
            # a stop inside a lens or a gap sits within factor `cut`, a propagation: the rear group starts behind it
            first = cut + 1 if cut + 1 < len(mats) and ends[cut] == ends[cut + 1] else cut
            rear = _chain(mats[first:])
            dist = ends[first] + self._v1 - z_s
            z_out = self._v2 + _conjugate(rear, dist)
            m_out = _between(rear, dist, z_out - self._v2)[0, 0]
        return float(z_in), float(z_out), float(m_in), float(m_out)

    def pupil_position(self, z_s: float) -> tuple:
        """z of the entrance and of the exit pupil of an aperture stop at z_s."""
        return self._pupils(z_s)[:2]

    def pupil_magnification(self, z_s: float) -> tuple:
        """Magnifications of the entrance and of the exit pupil of an aperture stop at z_s."""
        return self._pupils(z_s)[2:]
