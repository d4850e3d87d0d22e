# The wide cross-moments pass (xmom_wide_engine.hpp) on the null device, beside the drivers of Makefile:
#   xmom_wide_asan / xmom_wide_tsan                 the pass with its stand-in launcher
#   xmom_wide_absent_asan / xmom_wide_absent_tsan   the same with NO stand-in: FMHIP_ERR_UNSUPPORTED      tests/test_cross_moments_wide_cpu.py
include Makefile
$(call DRIVER,xmom_wide,null_xmom_wide)
$(call DRIVER,xmom_wide_absent,)
