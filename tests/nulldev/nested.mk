# Block moments and the repeat (nested_engine.hpp) on the null device, beside the drivers of Makefile:
#   nested_asan / nested_tsan                 the two calls with their stand-in launchers (null_nested.cpp sums the blocks phase by phase;
#                                             null_sort.cpp has the kernel that raises the flag)
#   nested_absent_asan / nested_absent_tsan   the same with NO stand-in for the nested kernels: FMHIP_ERR_UNSUPPORTED      tests/test_nested_cpu.py
include Makefile
$(call DRIVER,nested,null_nested null_sort)
$(call DRIVER,nested_absent,null_sort)
