# Block order statistics and the block sort (block_order_engine.hpp) on the null device, beside the drivers of Makefile:
#   block_order_asan / block_order_tsan                 the calls with their stand-in launcher (null_block_order.cpp sorts the padded keys and sums
#                                                       the ranges as a wave does; null_sort.cpp has the kernel that raises the flag)
#   block_order_absent_asan / block_order_absent_tsan   the same with NO stand-in for the kernel: FMHIP_ERR_UNSUPPORTED      tests/test_block_order_cpu.py
include Makefile
$(call DRIVER,block_order,null_block_order null_sort)
$(call DRIVER,block_order_absent,null_sort)
