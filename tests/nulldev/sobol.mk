# The Sobol' Brownian motion (fm_sobol_bm_kernel's launcher) on the null device under the sanitizers: make -f sobol.mk sobol_asan sobol_tsan
# (tests/test_sobol_device_cpu.py).  Everything else — the engine objects, the null device, the LINK rule — is the Makefile's, which stays
# as it is; the driver links null_sobol.cpp's stand-in and no other launcher.
include Makefile
# host/sobol.hpp is the definition for the host AND the device: no contraction into fused multiply-adds, wherever a compiler would
COMMON += -ffp-contract=off
HDRS   += $(HOSTDIR)/gamma_icdf.hpp $(HOSTDIR)/sobol.hpp $(HOSTDIR)/sobol_directions.hpp
$(call DRIVER,sobol,null_sobol)
