# The device sort (sort_engine.hpp) on the null device, beside the drivers of Makefile:
#   sort_asan / sort_tsan                 the four calls with their stand-in launchers (null_sort.cpp does the passes the plain way)
#   sort_absent_asan / sort_absent_tsan   the same with NO stand-in: FMHIP_ERR_UNSUPPORTED                  tests/test_sort_cpu.py
include Makefile
$(call DRIVER,sort,null_sort)
$(call DRIVER,sort_absent,)
