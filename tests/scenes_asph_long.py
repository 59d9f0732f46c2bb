"""Aspheres with more than OT_MAX_ASPH = 12 polynomial coefficients: the surfaces and the scene behind the fixtures
leaf_surfaces_asph_long.npz and trace_asphere_long*.npz (written by tests/golden/generate_golden_asph_long.py).  As in
tests/scenes.py every builder takes the package (`optrace` or `optrace_amd`) as its first argument.  An own file, so
that tests/scenes.py and the random streams of the older fixtures stay as they are."""
import numpy as np


def long_coeff(r, n, sign=1, A=1e-3):
    """a_j = sign A (-0.6)^j / r^(2j), j = 0 .. n-1: term j contributes sign A r^2 (-0.6)^j mm at the edge, a geometric
    series (smooth, monotone enough for the reference's geometry checks), and even the last of 32 terms still moves the
    edge by about 1e-7 A r^2 mm -- two orders above the position tolerance, so no coefficient can be dropped unnoticed."""
    j = np.arange(n)
    return list(sign * A * (-0.6) ** j / float(r) ** (2 * j))


def surface_zoo_long(ot):
    """n = 13, 16, 24 and 32 coefficients, both signs of R, k in {-2.5, -0.8, 0, 0.6}; one flipped after construction
    (negated coefficients, mirrored z range); one with 13 coefficients whose last one is 0.0 (the count counts)."""
    z = {}
    with ot.global_options.no_warnings():
        z["asph_n13"] = ot.AsphericSurface(r=2.5, R=8.0, k=-2.5, coeff=long_coeff(2.5, 13))
        z["asph_n16_neg"] = ot.AsphericSurface(r=3.0, R=-12.0, k=-0.8, coeff=long_coeff(3.0, 16, -1))
        z["asph_n24"] = ot.AsphericSurface(r=3.5, R=16.0, k=0.0, coeff=long_coeff(3.5, 24))
        z["asph_n32_neg"] = ot.AsphericSurface(r=4.0, R=-10.0, k=0.6, coeff=long_coeff(4.0, 32, -1))
        f = ot.AsphericSurface(r=3.0, R=10.0, k=-0.8, coeff=long_coeff(3.0, 16))
        f.flip()
        z["asph_n16_flipped"] = f
        z["asph_n13_last_zero"] = ot.AsphericSurface(r=2.5, R=-9.0, k=0.6, coeff=long_coeff(2.5, 12, -1) + [0.0])
    for j, (name, s) in enumerate(z.items()):
        s.move_to([0.07 * j - 0.2, 0.15 - 0.06 * j, 1.2 + 0.45 * j])
    return z


NAMES = ["asph_n13", "asph_n16_neg", "asph_n24", "asph_n32_neg", "asph_n16_flipped", "asph_n13_last_zero"]


def asphere_long_scene(ot, **rt_args):
    """A singlet whose front has 16 and whose back has 24 coefficients, a lens with a 3-coefficient aspheric front and a
    conic back (short and long aspheres in one scene and one kernel), a ring aperture, a rectangular detector; tilted
    Lambertian disc source so that some rays miss."""
    RT = ot.Raytracer(outline=[-8, 8, -8, 8, -12, 50], **rt_args)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.0), divergence="Lambertian", div_angle=12, pos=[0.3, -0.2, -10],
                        s=[0.02, 0.05, 1], spectrum=ot.LightSpectrum("Gaussian", mu=540., sig=40.),
                        polarization="Uniform"))
    with ot.global_options.no_warnings():
        front = ot.AsphericSurface(r=4, R=12, k=-0.8, coeff=long_coeff(4, 16))
        back = ot.AsphericSurface(r=4, R=-15, k=0.3, coeff=long_coeff(4, 24, -1))
        front2 = ot.AsphericSurface(r=3.5, R=9, k=-2.1, coeff=[1e-3, -2e-5, 2e-7])
    RT.add(ot.Lens(front, back, de=0.4, pos=[0, 0, 0],
                   n=ot.RefractionIndex("Sellmeier1", coeff=[1.03961212, 0.00600069867, 0.231792344,
                                                             0.0200179144, 1.01046945, 103.560653])))
    RT.add(ot.Lens(front2, ot.ConicSurface(r=3.5, R=-30, k=1.5), de=0.3, pos=[0, 0.1, 12],
                   n=ot.RefractionIndex("Abbe", n=1.6, V=45)))
    RT.add(ot.Aperture(ot.RingSurface(r=4.0, ri=1.6), pos=[0, 0, 17]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[8, 8]), pos=[0, 0, 30]))
    return RT
