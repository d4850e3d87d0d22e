# The transform option value per path (transform_engine.hpp) on the null device, beside the drivers of Makefile:
#   transform_asan / _tsan          fmhip_transform_option with its stand-in launcher (null_transform.cpp walks the groups the kernel's way)
#   transform_absent_asan / _tsan   the same with NO stand-in for the kernel: FMHIP_ERR_UNSUPPORTED      tests/test_transform_nulldev_cpu.py
include Makefile
$(call DRIVER,transform,null_transform)
$(call DRIVER,transform_absent,)
