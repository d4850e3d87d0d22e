# The polynomial regression in one pass (xmom_poly_engine.hpp) on the null device, beside the drivers of Makefile:
#   xmom_poly_asan / xmom_poly_tsan                 the two passes with their stand-in launchers
#   xmom_poly_absent_asan / xmom_poly_absent_tsan   the same with NO stand-in: FMHIP_ERR_UNSUPPORTED      tests/test_polynomial_regression_cpu.py
include Makefile
$(call DRIVER,xmom_poly,null_xmom_poly)
$(call DRIVER,xmom_poly_absent,)
