# The tabulated functions (table_engine.hpp) on the null device, beside the drivers of Makefile:
#   table_asan / table_tsan                 fmhip_table_apply with its stand-in launcher (null_table.cpp searches by the index the engine built)
#   table_absent_asan / table_absent_tsan   the same with NO stand-in for the kernel: FMHIP_ERR_UNSUPPORTED      tests/test_table_cpu.py
include Makefile
$(call DRIVER,table,null_table)
$(call DRIVER,table_absent,)
