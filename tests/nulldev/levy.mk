# The gamma / exponential increments (fm_mt_levy_kernel's launcher) on the null device under the sanitizers: make -f levy.mk levy_asan levy_tsan
# (tests/test_levy_increments_device_cpu.py).  Everything else — the engine objects, the null device, the LINK rule — is the Makefile's, which
# stays as it is; the driver links null_mt.cpp's stand-ins (jump, old laws) and null_mt_levy.cpp's.
include Makefile
# host/gamma_icdf.hpp is the definition of these laws for the host AND the device: no contraction into fused multiply-adds, wherever a compiler would
COMMON += -ffp-contract=off
HDRS   += $(HOSTDIR)/gamma_icdf.hpp
$(call DRIVER,levy,null_mt null_mt_levy)
