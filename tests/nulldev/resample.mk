# The device resampling (resample_engine.hpp) on the null device, beside the drivers of Makefile:
#   resample_asan / resample_tsan                 fmhip_resample with its stand-in launcher (null_resample.cpp walks the chunks and the tiles
#                                                 the kernels' way; null_sort.cpp has the kernel that raises the flag)
#   resample_absent_asan / resample_absent_tsan   the same with NO stand-in for the resample kernels: FMHIP_ERR_UNSUPPORTED      tests/test_resample_cpu.py
include Makefile
$(call DRIVER,resample,null_resample null_sort)
$(call DRIVER,resample_absent,null_sort)
