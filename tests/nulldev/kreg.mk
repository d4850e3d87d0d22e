# The kernel regression (kreg_engine.hpp) on the null device, beside the drivers of Makefile:
#   kreg_asan / kreg_tsan                 fmhip_kernel_moments with its stand-in launcher (null_kreg.cpp runs the definition)
#   kreg_absent_asan / kreg_absent_tsan   the same with NO stand-in for the kernel: FMHIP_ERR_UNSUPPORTED      tests/test_kernel_regression_cpu.py
include Makefile
$(call DRIVER,kreg,null_kreg)
$(call DRIVER,kreg_absent,)
