# The named functions and option formulas per path (analytic_engine.hpp) on the null device, beside the drivers of Makefile:
#   analytic_asan / analytic_tsan                 fmhip_function_apply and fmhip_option_formula with their stand-in launchers (null_analytic.cpp walks the groups the kernels' way)
#   analytic_absent_asan / analytic_absent_tsan   the same with NO stand-in for the kernels: FMHIP_ERR_UNSUPPORTED      tests/test_analytic_cpu.py
include Makefile
$(call DRIVER,analytic,null_analytic)
$(call DRIVER,analytic_absent,)
