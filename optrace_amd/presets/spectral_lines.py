"""Fraunhofer lines [nm] and the line triples used for Abbe numbers (presets/spectral_lines.py)."""

h = 404.6561    # Hg, violet
g = 435.8343    # Hg, blue
F_ = 479.9914   # Cd, blue (F')
F = 486.1327    # H, blue
e = 546.0740    # Hg, green
d = 587.5618    # He, yellow
D = 589.2938    # Na, yellow
C_ = 643.8469   # Cd, red (C')
C = 656.272     # H, red
r = 706.5188    # He, red
A_ = 768.2      # K, near infrared (A')

#: all lines, ordered by wavelength
all_lines = [h, g, F_, F, e, d, D, C_, C, r, A_]

FDC = [F, D, C]
FdC = [F, d, C]
FeC = [F, e, C]
F_eC_ = [F_, e, C_]
#: dominant wavelengths of the sRGB primaries, in the order b, g, r
rgb = [464.3118, 549.1321, 611.2826]

all_line_combinations = [FDC, FdC, FeC, F_eC_, rgb]
