# Order statistics across vectors and the selection behind their index (cross_order_engine.hpp) on the null device, beside the drivers of Makefile:
#   cross_order_asan / cross_order_tsan                 the calls with their stand-in launchers (null_cross_order.cpp sorts the padded words of a
#                                                       path with the kernels' network and walks the outputs as the kernel does)
#   cross_order_absent_asan / cross_order_absent_tsan   the same with NO stand-in for the kernels: FMHIP_ERR_UNSUPPORTED      tests/test_cross_order_cpu.py
include Makefile
$(call DRIVER,cross_order,null_cross_order)
$(call DRIVER,cross_order_absent,)
