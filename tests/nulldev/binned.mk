# The localized regression (fm_binned_xmom_kernel's and fm_binned_eval_kernel's launchers) on the null device under the sanitizers:
# make -f binned.mk binned_asan binned_tsan (tests/test_binned_device_cpu.py).  Everything else — the engine objects, the null device, the
# LINK rule — is the Makefile's, which stays as it is; the driver links null_binned.cpp's stand-ins and no other launcher.
include Makefile
# host/binned_regression.hpp is the definition for the host AND what the device is compared with: no contraction into fused multiply-adds
COMMON += -ffp-contract=off
HDRS   += $(HOSTDIR)/binned_regression.hpp
$(call DRIVER,binned,null_binned)
# … and a driver that links NO stand-in for the two launchers: the engine answers FMHIP_ERR_UNSUPPORTED
$(call DRIVER,binned_absent,)
