"""Refractive indices (medium_n of csrc/ot_device.hpp) and filter transmissions (filter_T) value by value: wavelengths,
media, filters, exact values and bars, shared by the fixture generator tests/golden/generate_golden_wavelength.py (run on the
reference), tests/test_wavelength_host.py and tests/test_gpu_wavelength_step.py.

Wavelengths (N_WL float32 values per case, no multiple of 64): 380 and 780 with their float32 neighbours inside the range,
the Fraunhofer lines the suite uses, for tables every node rounded to float32 with its float32 neighbours on both sides and
the midpoints between nodes, for filters their edges and the neighbours of those, and a random fill.  Built from the bit
generator with +, -, *, / alone.

Archive keys (tests/golden/wavelength_step.npz), per medium case `n/<case>` and filter case `T/<case>`:
  <key>/wl (N_WL,) f32       the wavelengths (a checksum of their own: the test regenerates and compares them)
  <key>/ref (N_WL,) f64      the reference's own value (RefractionIndex.__call__, TransmissionSpectrum.__call__ on the
                             float32 array, as the tracer calls them)
  <key>/hi (N_WL,) f64, /lo (N_WL,) f32    the same formula evaluated exactly (mpmath) on the binary values of the
                             coefficients, of the constants 1e-3, 0.028 and of the float32 wavelength
  gauss_ulp                  the reference's largest distance, in float32 units in the last place, from
                             fl32(val32 exp(q)) over all Gaussian cases (q from float32 basic operations, exp exact)

THE BARS
  bitwise   The reference's recorded value, on every route, for the models whose formula uses only correctly rounded
            operations in the reference's order (+ - * / sqrt): BITWISE_MEDIA, and the filter types Constant, Rectangle and
            Data.  Nothing to derive: IEEE arithmetic.
  powers    Cauchy, Conrady, Schott, Herzberger, Extended, Extended2, Extended3 contain x**k with k >= 3 (Conrady: 3.5), which
            NumPy hands to libm's pow, the host tables as well, and the device multiplies out.  Per sample, with u = 2^-53
            and the value written as [sqrt of] S = sum of terms t_j = c_j x^p_j over m terms:
                |S_computed - S| <= u sum_j |t_j| (e_j + m - 1)
                e_j = |p_j| r            r roundings in x itself: 2 for x = (wl 1e-3)^2, 1 for x = wl 1e-3
                    + 3                  where |p_j| >= 3: the three ulp the device's power documents (libm's is within one)
                    + |p_j| - 1          where 2 <= |p_j| < 3: the products
                    + 1                  the product with or the quotient by c_j (none for the constant term)
                m - 1                    every term passes through at most m - 1 additions
            and through the root, n = sqrt(S): |n_computed - n| <= |S_computed - S| / (2 n) + u n.  Herzberger's L =
            1 / (x - 0.028) has r_L = 2 x / (x - 0.028) + 2 roundings (the difference amplifies x's, then the difference and
            the quotient), and its terms e = r_L + 1 and 2 r_L + 2.  Evaluated in longdouble from the magnitudes of the exact
            terms (power_bound).  Every route has to be inside, and the host test asserts that the reference is.
  gaussian  T = val32 * exp(q), q = -(wl - mu32)^2 / den32 in float32 basic operations, which every machine reproduces;
            truth is fl32(val32 exp(q)) with exp exact.  The bar is max(2, gauss_ulp) float32 units: one for an expf faithful
            to one unit, one for the product; more only if the reference itself is measured farther off.  An inverse
            Gaussian is 1 - T: the bar's units are those of T (the subtraction is exact in double on the device, and
            rounds once more, 2^-25 absolute, in the reference's float32).
"""
from __future__ import annotations

import pathlib

import numpy as np

from focus_cases import write_npz  # noqa: F401
from refraction_cases import split, join  # noqa: F401

LD = np.longdouble
U = LD(2.0) ** -53
N_WL = 211
F32 = np.float32
FRAUNHOFER = (486.1327, 587.5618, 656.272, 479.9914, 546.0740, 643.8469, 589.2938, 435.8343, 706.5188)
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

BITWISE_MEDIA = ("Constant", "Abbe", "Sellmeier1", "Sellmeier2", "Sellmeier3", "Sellmeier4", "Sellmeier5",
                 "Handbook of Optics 1", "Handbook of Optics 2", "Data")
# model -> (variable, root, ((coefficient index, power of the variable), ...))
POWER_MEDIA = {
    "Cauchy": ("wl2", False, ((0, 0), (1, -1), (2, -2), (3, -3))),
    "Conrady": ("um", False, ((0, 0), (1, -1), (2, -3.5))),
    "Schott": ("wl2", True, ((0, 0), (1, 1), (2, -1), (3, -2), (4, -3), (5, -4))),
    "Extended": ("wl2", True, ((0, 0), (1, 1), (2, -1), (3, -2), (4, -3), (5, -4), (6, -5), (7, -6))),
    "Extended2": ("wl2", True, ((0, 0), (1, 1), (2, -1), (3, -2), (4, -3), (5, -4), (6, 2), (7, 3))),
    "Extended3": ("wl2", True, ((0, 0), (1, 1), (2, 2), (3, -1), (4, -2), (5, -3), (6, 4), (7, 5), (8, -6))),
    "Herzberger": ("wl2", False, None),
}
# one glass per model that the catalogue fixtures offer
AGF_GLASSES = (("misc.agf", "BASF5"), ("subset.agf", "SF5"), ("subset.agf", "N-SF5"), ("subset.agf", "J-LAF7"),
               ("subset.agf", "E-KZFH1"), ("subset.agf", "IRG2"), ("subset.agf", "AGASS3-E"), ("subset.agf", "AGGAS2-E"),
               ("subset.agf", "CALCITE"), ("subset.agf", "ZNO"), ("subset.agf", "KRS5"))


# ---- wavelengths --------------------------------------------------------------------------------------------------------
def _nb(x, up):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


def wavelengths(index: int, nodes=(), marks=(), lo=380.0, hi=780.0) -> np.ndarray:
    """nodes: table nodes (doubles); marks: other values whose float32 neighbourhood matters (filter edges, mu)."""
    out = [F32(380), _nb(380, True), F32(780), _nb(780, False)] + [F32(v) for v in FRAUNHOFER]
    nodes = np.asarray(nodes, dtype=np.float64)
    for v in list(nodes) + list(marks):
        c = F32(v)
        out += [c, _nb(c, False), _nb(c, True)]
    out += [F32((a + b) / 2) for a, b in zip(nodes[:-1], nodes[1:])]
    out = [v for v in out if lo <= float(v) <= hi]
    assert len(out) <= N_WL, len(out)
    rng = np.random.default_rng([20261, index])
    fill = (lo + (hi - lo) * rng.random(N_WL - len(out))).astype(F32)
    wl = np.concatenate((np.array(out, dtype=F32), np.clip(fill, F32(lo), F32(hi))))
    assert wl.shape[0] == N_WL and N_WL % 64 != 0
    return wl


# ---- media --------------------------------------------------------------------------------------------------------------
def uneven_nodes(lo: float, hi: float, step: float = 20.0) -> np.ndarray:
    """Nodes that are not equidistant and that both packages still accept (they refuse std(diff(wls)) > 1e-4): steps of
    20 nm with the inner nodes moved by +-2e-5 nm in turn, about one float32 spacing here, so that a node's float32
    neighbours and the midpoints fall on other sides of the nodes than in an equidistant table."""
    k = np.arange(int(round((hi - lo) / step)) + 1)
    wls = lo + step * k
    wls[1:-1] = wls[1:-1] + np.where(k[1:-1] % 2 == 0, 2e-5, -2e-5)
    return wls


def _tables() -> dict:
    k = np.arange(14)
    u = uneven_nodes(380.0, 780.0)
    return {
        "Data/uneven": dict(wls=u, vals=1.5 + 0.1 / (1 + np.arange(u.shape[0]) / 4.0) ** 2),
        "Data/two": dict(wls=np.array([380.0, 780.0]), vals=np.array([1.62, 1.58])),
        "Data/equal_pair": dict(wls=np.linspace(380.0, 780.0, 9), vals=np.array([1.7, 1.65, 1.65, 1.6, 1.58, 1.58, 1.58, 1.55, 1.5])),
        "Data/odd_nodes": dict(wls=380.0 + 400.0 * k / 13, vals=1.45 + 0.2 / (1 + k / 3.0)),   # no inner node is a float32
    }


def media_cases() -> dict:
    """case -> (n_type, kwargs); the catalogue glasses are filled in by medium() (they need the loader)."""
    import scenes
    out = {name: (name.split("_")[0], kw) for name, kw in scenes.MEDIA.items()}
    out.update({name: ("Data", kw) for name, kw in _tables().items()})
    out.update({f"agf/{glass}": (None, (file, glass)) for file, glass in AGF_GLASSES})
    return out


MEDIA_CASES = None


def media_names() -> list:
    global MEDIA_CASES
    if MEDIA_CASES is None:
        MEDIA_CASES = media_cases()
    return list(MEDIA_CASES)


def medium(ot, case: str):
    """The RefractionIndex of the case in either package (the catalogue glasses: read by the product's loader, then
    rebuilt in `ot` from type and coefficients, so no coefficient is typed in)."""
    media_names()
    n_type, kw = MEDIA_CASES[case]
    if n_type is None:
        import optrace_amd
        with optrace_amd.global_options.no_warnings():
            glass = optrace_amd.load_agf(str(GOLDEN / "load" / kw[0]))[kw[1]]
        return ot.RefractionIndex(glass.spectrum_type, coeff=list(glass.coeff))
    return ot.RefractionIndex(n_type, **kw)


def medium_wavelengths(case: str, ri) -> np.ndarray:
    nodes = np.asarray(ri._wls) if ri.spectrum_type == "Data" else ()
    return wavelengths(media_names().index(case), nodes=nodes)


# ---- filters ------------------------------------------------------------------------------------------------------------
FILTER_CASES = {
    "Constant": (dict(spectrum_type="Constant", val=0.6), ()),
    "Constant_inv": (dict(spectrum_type="Constant", val=0.6, inverse=True), ()),
    "Rectangle": (dict(spectrum_type="Rectangle", wl0=450.0, wl1=640.0, val=0.8), (450.0, 640.0)),
    "Rectangle_inv": (dict(spectrum_type="Rectangle", wl0=450.0, wl1=640.0, val=0.8, inverse=True), (450.0, 640.0)),
    "Rectangle_odd": (dict(spectrum_type="Rectangle", wl0=450.1, wl1=639.9, val=0.3), (450.1, 639.9)),   # edges no float32
    "Data": (dict(spectrum_type="Data", wls=np.linspace(400.0, 700.0, 31), vals=np.linspace(0.1, 0.9, 31) ** 2), "nodes"),
    "Data_inv": (dict(spectrum_type="Data", wls=np.linspace(400.0, 700.0, 31), vals=np.linspace(0.1, 0.9, 31) ** 2, inverse=True), "nodes"),
    "Data_uneven": (dict(spectrum_type="Data", wls=uneven_nodes(400.0, 700.0), vals=np.linspace(0.2, 0.95, 16) ** 2), "nodes"),
    "Gaussian60": (dict(spectrum_type="Gaussian", mu=550.0, sig=60.0, val=0.9), (550.0,)),
    "Gaussian5": (dict(spectrum_type="Gaussian", mu=550.123, sig=5.0, val=0.7), (550.123, 500.0, 600.0)),   # underflows to 0
    "Gaussian30_inv": (dict(spectrum_type="Gaussian", mu=500.0, sig=30.0, val=1.0, inverse=True), (500.0,)),
}
BITWISE_FILTERS = ("Constant", "Rectangle", "Data")


def filter_spectrum(ot, case: str):
    kw = dict(FILTER_CASES[case][0])
    return ot.TransmissionSpectrum(kw.pop("spectrum_type"), **kw)


def filter_wavelengths(case: str) -> np.ndarray:
    kw, marks = FILTER_CASES[case]
    nodes = kw["wls"] if marks == "nodes" else ()
    return wavelengths(1000 + list(FILTER_CASES).index(case), nodes=nodes, marks=() if marks == "nodes" else marks)


def weights(case_index: int) -> np.ndarray:
    """w0 of the rays of a filter launch: the first half 1 and 0.5 in turn (the stored weight is fl32(T) or half of it
    exactly), the rest random float32 (the product's two roundings, (float)((double)w * T))."""
    rng = np.random.default_rng([20262, case_index])
    w = (0.25 + 0.75 * rng.random(N_WL)).astype(F32)
    w[:N_WL // 2:2], w[1:N_WL // 2:2] = 1.0, 0.5
    return w


# ---- Function spectra ---------------------------------------------------------------------------------------------------
def index_function(wl):
    return 1.5 + 4000.0 / (wl * wl) + 1e-5 * np.sqrt(wl)


def transmission_function(wl):
    return 0.25 + 0.5 * (wl - 380.0) / 400.0


FUNCTION_GRID = 65537   # nodes of the table a Function spectrum becomes under a continuous source


def function_table(func, inverse=False):
    """The table of a Function spectrum under a continuous source (RefractionIndex._desc, TransmissionSpectrum._desc):
    the function on 65537 equidistant nodes, an inverse filter folded in as 1 - f."""
    x = np.linspace(380.0, 780.0, FUNCTION_GRID)
    v = np.asarray(func(x), dtype=np.float64)
    return x, (1.0 - v if inverse else v)


def function_wavelengths() -> np.ndarray:
    """Nodes of the fine table (every one a float32: multiples of 2^-12), their float32 neighbours, midpoints, a fill."""
    x = np.linspace(380.0, 780.0, FUNCTION_GRID)
    nodes = x[[0, 1, 2, 3, 1000, 1001, 1002, 21845, 21846, 32767, 32768, 32769, 43690, 43691, 60000, 60001, 65533, 65534, 65535, 65536]]
    assert np.all(nodes.astype(F32) == nodes)
    return wavelengths(998, nodes=nodes)


# ---- exact values ---------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.prec = 300
    return mpmath


def exact_index(model: str, c, wl32, table=None):
    """The formula of refraction_index.py:83-162 exactly, on the binary values.  c: the coefficients as the device record
    holds them (Abbe: A, B, d).  table: (wls, vals) for Data."""
    mp = _mp()
    f = mp.mpf
    c = [f(float(v)) for v in c]
    um = f(float(wl32)) * f(1e-3)
    x = um * um
    if model == "Constant":
        return c[0]
    if model == "Abbe":
        return c[0] + c[1] / (x - c[2])
    if model == "Sellmeier1":
        return mp.sqrt(1 + c[0] * x / (x - c[1]) + c[2] * x / (x - c[3]) + c[4] * x / (x - c[5]))
    if model == "Sellmeier2":
        return mp.sqrt(1 + c[0] + c[1] * x / (x - c[2] ** 2) + c[3] / (x - c[4] ** 2))
    if model == "Sellmeier3":
        return mp.sqrt(1 + sum(c[2 * j] * x / (x - c[2 * j + 1]) for j in range(4)))
    if model == "Sellmeier4":
        return mp.sqrt(c[0] + c[1] * x / (x - c[2]) + c[3] * x / (x - c[4]))
    if model == "Sellmeier5":
        return mp.sqrt(1 + sum(c[2 * j] * x / (x - c[2 * j + 1]) for j in range(5)))
    if model == "Handbook of Optics 1":
        return mp.sqrt(c[0] + c[1] / (x - c[2]) - c[3] * x)
    if model == "Handbook of Optics 2":
        return mp.sqrt(c[0] + c[1] * x / (x - c[2]) - c[3] * x)
    if model == "Herzberger":
        L = 1 / (x - f(0.028))
        return c[0] + c[1] * L + c[2] * L ** 2 + c[3] * x + c[4] * x ** 2 + c[5] * x ** 3
    if model in POWER_MEDIA:
        var, root, terms = POWER_MEDIA[model]
        v = x if var == "wl2" else um
        S = sum(c[j] * mp.power(v, f(p)) for j, p in terms)
        return mp.sqrt(S) if root else S
    if model == "Data":
        return exact_interp(float(wl32), *table)
    raise ValueError(model)


def exact_interp(x, xp, fp):
    """Linear interpolation exactly; 0 outside the table (the filters' left and right)."""
    mp = _mp()
    f = mp.mpf
    if x < xp[0] or x > xp[-1]:
        return f(0)
    j = int(np.searchsorted(xp, x, side="right")) - 1
    if j == len(xp) - 1:
        return f(float(fp[j]))
    return f(float(fp[j])) + (f(float(fp[j + 1])) - f(float(fp[j]))) / (f(float(xp[j + 1])) - f(float(xp[j]))) * (f(x) - f(float(xp[j])))


def gaussian_q(wl32, mu, sig) -> np.ndarray:
    """-(wl - mu)^2 / (2 sig^2) as NumPy forms it on a float32 array (spectrum.py:112): float32 basic operations."""
    wl32 = np.asarray(wl32, dtype=F32)
    d = wl32 - F32(mu)
    return -(d * d) / F32(2 * sig ** 2)


def exact_transmission(kw: dict, wl32):
    """-> mpf; for the Gaussian fl32(val32 exp(q)) as an mpf (the truth of the bar), 1 - that for an inverse one."""
    mp = _mp()
    f = mp.mpf
    st, wl = kw["spectrum_type"], float(wl32)
    if st == "Constant":
        T = f(float(kw["val"]))
    elif st == "Rectangle":
        T = f(float(kw["val"])) if kw["wl0"] <= wl <= kw["wl1"] else f(0)
    elif st == "Data":
        T = exact_interp(wl, kw["wls"], kw["vals"])
    elif st == "Gaussian":
        q = float(gaussian_q(np.array([wl32], dtype=F32), kw["mu"], kw["sig"])[0])
        T = f(float(F32(float(f(float(F32(kw["val"]))) * mp.exp(f(q))))))
    else:
        raise ValueError(st)
    return 1 - T if kw.get("inverse") else T


# ---- bars -----------------------------------------------------------------------------------------------------------------
def model_of(ri) -> str:
    return ri.spectrum_type


def coefficients(ri) -> list:
    """The numbers the formula is evaluated on: c of the device record (Abbe: A, B, d)."""
    if ri.spectrum_type == "Constant":
        return [float(ri.val)]
    if ri.spectrum_type == "Abbe":
        return list(ri._abbe_AB())
    return [] if ri.coeff is None else [float(v) for v in ri.coeff]


def power_bound(model: str, c, wl32) -> np.ndarray:
    """The forward error bound of the module docstring for every wavelength, in longdouble."""
    um = np.asarray(wl32, dtype=F32).astype(LD) * LD(1e-3)
    x = um * um
    c = [LD(v) for v in c]
    if model == "Herzberger":
        L = 1 / (x - LD(0.028))
        rL = 2 * x / (x - LD(0.028)) + 2
        terms = [(c[0] + 0 * x, 0 * x), (c[1] * L, rL + 1), (c[2] * L * L, 2 * rL + 2), (c[3] * x, 2 + 1 + 0 * x),
                 (c[4] * x * x, 4 + 1 + 1 + 0 * x), (c[5] * x * x * x, 6 + 3 + 1 + 0 * x)]
        root = False
    else:
        var, root, spec = POWER_MEDIA[model]
        v, r = (x, 2) if var == "wl2" else (um, 1)
        terms = []
        for j, p in spec:
            a = abs(p)
            e = a * r + (3 if a >= 3 else max(a - 1, 0)) + (1 if p != 0 else 0)
            terms.append((c[j] * v ** LD(p), e + 0 * x))
    m = len(terms)
    S = sum(t for t, _ in terms)
    err = U * sum(np.abs(t) * (e + m - 1) for t, e in terms)
    if root:
        n = np.sqrt(S)
        return err / (2 * n) + U * n
    return err


def ulp32(a, b) -> np.ndarray:
    """Distance of two float32 arrays of non-negative values in units of the last place."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def gaussian_bar(g) -> int:
    return max(2, int(g["gauss_ulp"]))


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def index_report(case: str, ri, wl, g, got, route: str) -> tuple:
    """One route's indices `got` (f64) against the bar of the case's model -> (line for the log, passes)."""
    model, ref = model_of(ri), g[f"n/{case}/ref"]
    truth = join(g[f"n/{case}/hi"], g[f"n/{case}/lo"])
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - truth)
    if model in POWER_MEDIA:
        ratio = float(np.max(err / power_bound(model, coefficients(ri), wl)))
        return f"{route:10s} n {case:24s} {model:22s} largest error / bar {ratio:.3f}, {float(err.max()):.2e} abs", ratio <= 1
    same = bits(np.asarray(got, dtype=np.float64), ref)
    off = int(np.count_nonzero(np.asarray(got, dtype=np.float64) != ref))
    return f"{route:10s} n {case:24s} {model:22s} bitwise: {off} of {wl.shape[0]} differ, {float(err.max()):.2e} from the truth", same


def transmission_report(case: str, g, got, route: str) -> tuple:
    """One route's transmissions `got` (f64) against the case's bar."""
    kw, ref = FILTER_CASES[case][0], g[f"T/{case}/ref"]
    got = np.asarray(got, dtype=np.float64)
    truth = g[f"T/{case}/hi"]
    if kw["spectrum_type"] != "Gaussian":   # (a route shows T through a float32 weight: w0 = 1 gives fl32(T))
        off = int(np.count_nonzero(got.astype(F32) != ref.astype(F32)))
        return f"{route:10s} T {case:24s} bitwise: {off} of {got.shape[0]} differ", bits(got.astype(F32), ref.astype(F32))
    bar = gaussian_bar(g)
    if kw.get("inverse"):
        T, Tt = 1 - got, 1 - truth
        unit = np.spacing(Tt.astype(F32)).astype(np.float64)
        worst = float(np.max(np.maximum(np.abs(T - Tt) - 2.0 ** -25, 0) / unit))
        ok = bool(np.all(np.abs(T - Tt) <= bar * unit + 2.0 ** -25))
        return f"{route:10s} T {case:24s} 1 - T: {worst:.2f} float32 units of T beyond the 2^-25 of the last rounding (bar {bar})", ok
    assert np.all(got.astype(F32) == got)
    d = ulp32(got, truth)
    zeros = np.array_equal(got == 0, ref == 0)
    return (f"{route:10s} T {case:24s} largest distance {int(d.max())} float32 units (bar {bar}), zeros where the reference's: {zeros}",
            bool(d.max() <= bar) and zeros)
