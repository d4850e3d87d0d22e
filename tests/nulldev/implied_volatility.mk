# The implied volatility per path (implied_volatility_engine.hpp) on the null device, beside the drivers of Makefile:
#   implied_volatility_asan / _tsan          fmhip_implied_volatility with its stand-in launcher (null_implied_volatility.cpp walks the groups the kernel's way)
#   implied_volatility_absent_asan / _tsan   the same with NO stand-in for the kernel: FMHIP_ERR_UNSUPPORTED      tests/test_implied_volatility_cpu.py
include Makefile
$(call DRIVER,implied_volatility,null_implied_volatility)
$(call DRIVER,implied_volatility_absent,)
