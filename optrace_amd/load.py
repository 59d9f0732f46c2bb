"""Import of ZEMAX files: `.agf` glass catalogues and `.zmx` lens prescriptions (optrace/tracer/load.py:57-415).

Host-only: text in, `RefractionIndex` objects and a `Group` out.  Nothing here touches the device -- the plausibility
check of a catalogue entry evaluates its formula at three wavelengths in float64 on the host
(`refraction_index.index_at`), so a catalogue of several hundred glasses loads without a single device call and on a
machine without a GPU.

File formats: ZEMAX Optical Design Program User's Manual (July 8, 2011), chapter "Using Glass Catalogs" for `.agf`;
User's Guide version 9.0, chapter 29 "The ZMX file format" for `.zmx`.  Of a catalogue record the lines
    NM <name> <formula number> <..> <n at the centre line> <Abbe number> ...
    CD <coefficient> ...
    LD <shortest> <longest wavelength of validity, in micrometres>
are read; of a prescription the header keys NAME, UNIT, MODE and per SURF block the keys TYPE, DIAM, CONI, COMM, COAT,
STOP, CURV, DISZ, PARM and GLAS, which stand in columns 2-6 of their lines.

Text encoding is decided by the byte-order mark (UTF-8, UTF-16, UTF-32); a file without one is UTF-8 if it decodes as
such, else Latin-1.  (The reference asks the `chardet` package, a statistical guess.)
"""
from __future__ import annotations

import codecs
import os.path

import numpy as np

from ._warn import warning
from .geometry import (Group, Lens, Aperture, Detector, PointMarker, Surface, CircularSurface, SphericalSurface,
                       ConicSurface, AsphericSurface, RingSurface, RectangularSurface)
from .presets import spectral_lines
from .refraction_index import RefractionIndex, index_at, abbe_at

#: formula number of an `.agf` record (1-13) -> n_type of RefractionIndex
_AGF_FORMULAS = ("Schott", "Sellmeier1", "Herzberger", "Sellmeier2", "Conrady", "Sellmeier3", "Handbook of Optics 1",
                 "Handbook of Optics 2", "Sellmeier4", "Extended", "Sellmeier5", "Extended2", "Extended3")

INDEX_TOLERANCE = 1e-4  #: |n from the formula - n stated in the record| above which `load_agf` warns
ABBE_TOLERANCE = 0.3    #: the same for the Abbe number
CEMENT_GAP = 1e-7       #: [mm] by which a lens cemented to the one before it starts behind that lens' back surface

# (UTF-32 first: its little-endian mark starts with the UTF-16 one)
_MARKS = ((codecs.BOM_UTF32_LE, "utf-32"), (codecs.BOM_UTF32_BE, "utf-32"), (codecs.BOM_UTF8, "utf-8-sig"),
          (codecs.BOM_UTF16_LE, "utf-16"), (codecs.BOM_UTF16_BE, "utf-16"))


def _read_lines(path: str) -> list:
    """Lines of a text file (line ends kept as "\\n"), decoded by the rule in the module's description."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found/ is not a file.")
    with open(path, "rb") as f:
        raw = f.read()
    encoding = next((enc for mark, enc in _MARKS if raw.startswith(mark)), None)
    if encoding is None:
        try:
            raw.decode("utf-8")
            encoding = "utf-8"
        except UnicodeDecodeError:
            encoding = "latin-1"
    parts = raw.decode(encoding).replace("\r\n", "\n").replace("\r", "\n").split("\n")
    return [part + "\n" for part in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


# ---- glass catalogues ---------------------------------------------------------------------------------------------
def _checked_medium(name: str, mode: str, coeff: list, nc: float, V: float, wl0: float, wl1: float) -> RefractionIndex:
    """The medium of one catalogue record; warns where the formula and the record's own n and V disagree."""
    n = RefractionIndex(mode, coeff=coeff, desc=name)
    F, d, C = spectral_lines.FdC
    if wl0 > F or wl1 < C:
        warning(f"{name} wavelength range [{wl0}, {wl1}]nm does not overlap with "
                f"testing wavelengths {spectral_lines.FdC}nm, skipping index and Abbe number checks.")
        return n
    nc1 = index_at(n, d)
    V1 = abbe_at(n, spectral_lines.FdC)
    if abs(nc1 - nc) > INDEX_TOLERANCE:
        warning(f"{name}: Index from file is {nc}, but calculated index is {nc1}. "
                "This can be due to different probe wavelengths.")
    elif abs(V1 - V) > ABBE_TOLERANCE:
        warning(f"{name}: The Abbe number from file is {V}, but calculated is {V1}. "
                "This can be due to different probe wavelengths.")
    return n


def load_agf(path: str) -> dict:
    """Load an .agf material catalogue.

    :param path: filepath
    :return: dictionary of refractive media, keys are names, values are RefractionIndex objects
    """
    media = {}
    rec = None  # the record being read: name, mode, nc, V, coeff; None while a record is skipped
    for line in _read_lines(path):
        tag = line[:2]
        if tag == "NM":
            words = line.split()
            name, number = words[1], int(float(words[2]))
            if not 1 <= number <= len(_AGF_FORMULAS):
                warning(f"{name}: Unknown index formula mode number {number}, skipping.")
                rec = None
                continue
            rec = dict(name=name, mode=_AGF_FORMULAS[number - 1], nc=float(words[4]), V=float(words[5]), coeff=None)
        elif tag == "CD" and rec is not None:
            given = [float(w) for w in line.split()[1:]]
            count = RefractionIndex.coeff_count[rec["mode"]]
            rec["coeff"] = (given + [0.] * count)[:count]  # cut, or padded with zeros
        elif tag == "LD" and rec is not None:  # the validity range closes a record
            try:
                lo, hi = (float(w) * 1000 for w in line.split()[1:3])
                media[rec["name"]] = _checked_medium(rec["name"], rec["mode"], rec["coeff"], rec["nc"], rec["V"], lo, hi)
            except Exception as err:  # noqa: BLE001 - whatever is wrong with one glass (n < 1, ...), the others load
                warning(f"Error for material {rec['name']}: " + str(err))
    return media


# ---- prescriptions ------------------------------------------------------------------------------------------------
def _header(lines: list) -> tuple:
    """(description, index of the first SURF line) of a prescription; refuses units and modes that are not supported."""
    desc = ""
    for i, line in enumerate(lines):
        key = line[:4]
        if key == "NAME":
            desc = line[5:-1]
        elif key == "UNIT":
            unit = line.split()[1]
            if unit != "MM":
                raise RuntimeError(f"Unsupported Unit {unit}.")
        elif key == "MODE":
            mode = line.split()[1]
            if mode != "SEQ":
                raise RuntimeError(f"Unsupported Mode {mode}.")
        elif key == "SURF":
            return desc, i
    return desc, len(lines) - 1


def _blocks(lines: list, first: int) -> list:
    """The property lines of every SURF block behind line `first`.  The last line of the file closes the last block
    and is not read as a property."""
    if first + 1 >= len(lines):
        return []
    blocks = [[]]
    for line in lines[first + 1:-1]:
        if line[:4] == "SURF":
            blocks.append([])
        else:
            blocks[-1].append(line)
    return blocks


def _glass(words: list, n_dict: dict) -> RefractionIndex:
    """Medium of a GLAS line: from the catalogue, or an Abbe model where the line itself states n and V."""
    material = words[1]
    nc, V = (float(w) for w in words[4:6]) if len(words) > 6 else (None, None)
    if material == "___BLANK":
        return RefractionIndex("Abbe", n=nc, V=V)
    if material in n_dict:
        return n_dict[material]
    if nc is not None and nc > 1 and V > 0:
        return RefractionIndex("Abbe", n=nc, V=V)
    raise RuntimeError(f"Material {material} missing in n_dict parameter.")


def _surface_record(block: list, n_dict: dict) -> tuple:
    """(properties, distance to the next surface) of one SURF block."""
    surf = dict(stype="STANDARD", desc="", k=0, R=np.inf, parm=[0.] * 10)
    dist = 0
    for line in block:
        key, words = line[2:6], line.split()
        if key == "TYPE":
            surf["stype"] = words[1]
        elif key == "DIAM":
            surf["r"] = max(float(words[1]), 1e-9)
        elif key == "CONI":
            surf["k"] = float(words[1])
        elif key == "COMM":
            surf["desc"] = line[7:-1]
        elif key == "COAT":
            warning(f"Coatings are not supported. Ignoring coating '{line[7:-1]}'.")
        elif key == "STOP":
            surf["STOP"] = True
        elif key == "CURV":
            curvature = float(words[1])
            surf["R"] = 1 / curvature if curvature else np.inf
        elif key == "DISZ":
            dist = max(float(words[1]), 3 * Surface.N_EPS)  # surfaces must not touch
        elif key == "PARM":
            surf["parm"][int(float(words[1])) - 1] = float(words[2])
        elif key == "GLAS":
            surf["n"] = _glass(words, n_dict)
    return surf, dist


def _make_surface(surf: dict) -> Surface:
    """Surface object of a surface record: STANDARD is a disc, a sphere or a conic, EVENASPH an asphere."""
    kind, r, R, desc = surf["stype"], surf["r"], surf["R"], surf["desc"]
    if kind == "STANDARD":
        if not np.isfinite(R):
            return CircularSurface(r=r, desc=desc)
        if surf["k"]:
            return ConicSurface(r=r, R=R, k=surf["k"], desc=desc)
        return SphericalSurface(r=r, R=R, desc=desc)
    if kind == "EVENASPH":
        return AsphericSurface(r=r, R=R, k=surf["k"], coeff=surf["parm"], desc=desc)
    raise RuntimeError("Surface mode " + str(kind) + " not supported yet.")


def _assemble(surfaces: list, dists: list, n0, long_desc: str, no_marker: bool) -> Group:
    """Group of lenses, stop and detector from the surface records.

    A surface with a medium opens a lens that the next surface closes.  If that next surface has a medium too, the two
    lenses are cemented: the surface is built twice, as the back of the one lens and, CEMENT_GAP further on, as the
    front of the next, with the first lens' medium in the gap.  Surfaces without a medium between lenses are the stop
    (a ring aperture) or, at the very end, the image plane (a square detector); before the first lens they are skipped.
    """
    G = Group(long_desc=long_desc, n0=n0)
    known = [s["r"] for s in surfaces if "r" in s]
    widest = max(known, default=0)
    for s in surfaces:  # a medium that extends sideways without bound has no radius in the file
        s.setdefault("r", widest)

    i = next((j for j, s in enumerate(surfaces) if "n" in s), len(surfaces))
    z = 0
    while i < len(surfaces):
        s = surfaces[i]
        if "n" not in s:
            if i + 1 == len(surfaces):
                side = 2 * s["r"]
                G.add(Detector(RectangularSurface(dim=[side, side]), pos=[0, 0, z], desc=s["desc"]))
            elif "STOP" in s:
                ext = G.extent
                outer = max(s["r"] + 1, max(ext[1] - ext[0], ext[3] - ext[2]) / 2)
                G.add(Aperture(RingSurface(ri=s["r"], r=outer), pos=[0, 0, z], desc=s["desc"]))
            z += dists[i]
            i += 1
            continue

        nxt = surfaces[i + 1]
        cemented = "n" in nxt
        n2 = s["n"] if cemented else RefractionIndex("Constant", n=1)
        G.add(Lens(_make_surface(s), _make_surface(nxt), n=s["n"], pos=[0, 0, z], d1=0, d2=dists[i], n2=n2,
                   desc=s["desc"]))
        if cemented:
            z += dists[i] + CEMENT_GAP
            i += 1
        else:
            z += dists[i] + dists[i + 1]
            i += 2

    if G.long_desc != "" and not no_marker:  # the description as a label beside the system
        ext = G.extent
        G.add(PointMarker(G.long_desc, [ext[0] - 1.5, np.mean(ext[2:4]), np.mean(ext[4:6])], label_only=True))
    return G


def load_zmx(filename: str, n_dict: dict = None, no_marker: bool = False) -> Group:
    """Load a ZEMAX geometry from a .zmx into a Group.  Sequential mode, millimetres, STANDARD and EVENASPH surfaces;
    coatings are ignored with a warning, tilts and decentres are not read.

    :param filename: filepath
    :param n_dict: dictionary of RefractionIndex for the glass names in the file
    :param no_marker: if there should be no marker created for the .zmx description
    :return: Group including the geometry from the .zmx
    """
    lines = _read_lines(filename)
    n_dict = n_dict or {}
    long_desc, first = _header(lines)

    surfaces, dists, n0 = [], [], None
    for number, block in enumerate(_blocks(lines, first)):
        surf, dist = _surface_record(block, n_dict)
        if number == 0 and not np.isfinite(dist):  # the object at infinity: its medium is the ambient one
            n0 = surf.get("n", RefractionIndex("Constant", n=1))
        else:
            surfaces.append(surf)
            dists.append(dist)
    return _assemble(surfaces, dists, n0, long_desc, no_marker)
