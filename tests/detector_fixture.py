"""Reader of tests/golden/detectors.npz (written by tests/golden/generate_golden_detectors.py): the reference's detector
hits for every detector kind at every placement, stored as a few concatenated arrays."""
from __future__ import annotations

import functools

import numpy as np

import scenes
from helpers import load


class DetectorFixture:
    def __init__(self):
        g = load("detectors.npz")
        self.g = {k: g[k] for k in g.files}
        self._rec = {str(k): j for j, k in enumerate(self.g["rec/keys"])}
        self._img = {str(k): j for j, k in enumerate(self.g["img/keys"])}
        self._rec_off = np.concatenate(([0], np.cumsum(self.g["rec/n"])))
        self._img_off = np.concatenate(([0], np.cumsum(self.g["img/n"])))

    def scene(self, name: str) -> dict:
        """N, p0, s0, pol0 (None without polarisation), w0, wl, N_list, p_list, w_list of a fixture scene"""
        d = {k.split("/", 1)[1]: v for k, v in self.g.items() if k.startswith(name + "/")}
        d.setdefault("pol0", None)
        return d

    def record(self, key: str) -> dict:
        j = self._rec[key]
        a, b = self._rec_off[j], self._rec_off[j + 1]
        g = self.g
        return dict(pos=g["rec/pos"][j], extent=g["rec/extent"][j], ill=int(g["rec/ill"][j]), ph=g["rec/ph"][a:b],
                    w=g["rec/w"][a:b], wl=g["rec/wl"][a:b])

    def image(self, key: str) -> dict:
        """uext (None for the automatic extent), extent, power, dense (Ny, Nx, 4) image"""
        j = self._img[key]
        a, b = self._img_off[j], self._img_off[j + 1]
        g = self.g
        dense = np.zeros(tuple(g["img/shape"][j]))
        dense[g["img/iy"][a:b], g["img/ix"][a:b]] = g["img/val"][a:b]
        uext = g["img/uext"][j]
        return dict(uext=None if np.isnan(uext[0]) else uext, extent=g["img/extent"][j], power=float(g["img/power"][j]),
                    dense=dense)


@functools.lru_cache(maxsize=1)
def fixture() -> DetectorFixture:
    return DetectorFixture()


def records(scene: str = None) -> list:
    """(scene, kind, placement, projection) of every record (of one scene)"""
    return [(name, *rec) for name in scenes.DETECTOR_SCENES if scene in (None, name) for rec in scenes.detector_records(name)]


def record_id(rec) -> str:
    return "/".join(str(v) for v in rec)
