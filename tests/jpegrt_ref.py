"""The JPEG round trip in numpy (PARITY_ASSUMPTIONS.md row 20): the pixels the JPEG of an image at
quality Q decodes to at scale 1/s.  No arithmetic of its own: tests/jpegc_ref.py (row 17), then
tests/jpegd_ref.py or tests/jpegds_ref.py (rows 18, 19) on those coefficients with that quality's
tables, then tests/ycc_ref.py (row 16).  tests/test_jpegrt_cpu.py pins the composition to
libjpeg-turbo's encode -> decode inside Pillow; the GPU tests hold MIPX_OP_JPEGRT to it.  Not part
of the oracle."""
import numpy as np

from jpegc_ref import jpegc_ref, qtables
from jpegd_ref import YCC_420, YCC_444, jpegd_ref, payload  # noqa: F401
from jpegds_ref import jpegds_ref, out_size
from ycc_ref import ycc_ref


def jpegrt_ref(rgb, layout, quality, s=1, trace=None):
    """rgb (h, w, 3) or (n, h, w, 3) uint8 -> (n, ceil(h / s), ceil(w / s), 3) uint8."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    if rgb.ndim == 3:
        rgb = rgb[None]
    _, h, w, _ = rgb.shape
    p = np.stack([payload(c, qtables(quality)) for c in jpegc_ref(rgb, layout, quality)])
    if s == 1:   # the file's own sampling: 4:2:0 chroma is upsampled
        return ycc_ref(jpegd_ref(p, w, h, layout, trace), w, h, layout)
    ow, oh = out_size(w, h, s)
    return ycc_ref(jpegds_ref(p, w, h, layout, s, trace), ow, oh, YCC_444)
