# The device selection (select_engine.hpp) on the null device, beside the drivers of Makefile:
#   select_asan / select_tsan                 fmhip_compress, fmhip_expand and fmhip_gather with their stand-in launchers (null_select.cpp walks
#                                             the chunks and the tiles the kernels' way; null_sort.cpp has the kernel that raises the flag)
#   select_absent_asan / select_absent_tsan   the same with NO stand-in for the selection kernels: FMHIP_ERR_UNSUPPORTED      tests/test_select_cpu.py
include Makefile
$(call DRIVER,select,null_select null_sort)
$(call DRIVER,select_absent,null_sort)
