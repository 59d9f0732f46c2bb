// trace_kernel variants of feature level OT_FEAT(OT_HIT_SPLINE, 1) (ot_trace_kernel.hpp)
#include "ot_trace_kernel.hpp"

OT_DEFINE_TRACE_UNIT(OT_FORM_STORE, OT_FEAT(OT_HIT_SPLINE, 1))
