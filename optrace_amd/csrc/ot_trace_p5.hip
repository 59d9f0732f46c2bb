// trace_pol_kernel variants (the polarisation planes replayed, ot_rays_fill_pol) of feature level OT_FEAT(OT_HIT_SPLINE, 1) (ot_trace_kernel.hpp)
#include "ot_trace_kernel.hpp"

OT_DEFINE_TRACE_UNIT(OT_FORM_POL, OT_FEAT(OT_HIT_SPLINE, 1))
