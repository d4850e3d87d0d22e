# The device reduce-by-key (group_engine.hpp) on the null device, beside the drivers of Makefile:
#   group_asan / group_tsan                 fmhip_group_sums with its stand-in launchers (null_group.cpp scans chunk by chunk with a carry, the
#                                           kernels' way; null_sort.cpp has the radix passes and the kernel that raises the flag)
#   group_absent_asan / group_absent_tsan   the same with NO stand-in for the group kernels: FMHIP_ERR_UNSUPPORTED        tests/test_group_cpu.py
include Makefile
$(call DRIVER,group,null_group null_sort)
$(call DRIVER,group_absent,null_sort)
