# The device prefix sums (prefix_engine.hpp) on the null device, beside the drivers of Makefile:
#   prefix_asan / prefix_tsan                 the three calls with their stand-in launchers (null_prefix.cpp scans the chunks the plain way;
#                                             null_sort.cpp has the kernel that raises the flag)
#   prefix_absent_asan / prefix_absent_tsan   the same with NO stand-in for the prefix kernels: FMHIP_ERR_UNSUPPORTED      tests/test_prefix_cpu.py
include Makefile
$(call DRIVER,prefix,null_prefix null_sort)
$(call DRIVER,prefix_absent,null_sort)
