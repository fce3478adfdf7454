"""imaginary_amd — MI355X-native pixel-transform engine for imaginary's hot path.

The product is libmipx.so (gfx950 HIP kernels + C-ABI, include/mipx.h); this
package is its Python binding plus a mirror of imaginary's operation layer.
Importing it fails when libmipx.so has not been built: there is no CPU path.
"""
from ._abi import lib, MipxError, MipxPlan, MipxOpts, MipxInput, LIB_PATH, TYPES, EXTEND, GRAVITY  # noqa: F401
from ._abi import (MIPX_OK, MIPX_EINVAL, MIPX_EUNSUPPORTED, MIPX_ENOMEM, MIPX_ENODEV, MIPX_EDEVICE,  # noqa: F401
                   MIPX_ETIMEOUT, MIPX_ENOTINIT, MIPX_ESTALE, MIPX_EBUSY)
from .engine import (DeviceBuffer, Engine, GuardedBuffer, device_count, execute, fit_dimension,  # noqa: F401
                     guard_damage, guard_setting, guarded_calls, make_input, make_opts, plan_add_textmark, plan_chain,
                     plan_make, plan_textmark_geometry, reduce_sampling, run_op, set_guard, set_reduce_sampling,
                     smartcrop_origins, synchronize, plan_set_ycc_input, ycc_bytes, ycc_to_rgb, YCC_444, YCC_420, YCC_422, YCC_GREY,
                     plan_set_jpegc_output, jpegc_bytes, jpeg_qtables, rgb_to_jpegc,
                     plan_set_jpegd_input, plan_set_jpegd_input_scaled, jpegd_bytes, jpegd_to_rgb,
                     jpegd_to_rgb_scaled, plan_add_jpeg_roundtrip, jpeg_roundtrip,
                     plan_set_jpeg_scan_output, jpeg_scan_bytes, jpeg_scan_opt_bytes, rgb_to_jpeg_scan, jpegc_to_scan, scan_slot,
                     rgb_to_jpeg_scan_packed, jpegc_to_scan_packed, scan_unpack,
                     jpegh_bytes, plan_set_jpegh_input, plan_set_jpegh_input_scaled, execute_status, jpegh_to_jpegd, jpegh_to_rgb, jpegh_to_rgb_scaled, JPEGH_OK, JPEGH_UNSYNCED,
                     JPEGH_BAD)

__version__ = "0.2.0"
