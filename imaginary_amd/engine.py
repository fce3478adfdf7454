"""Thin Python handle on libmipx.so: device buffers, per-op calls, plan execution.

Everything here calls the HIP library through the C-ABI; there is no CPU
compute path.  Used by the tests, smoke() and bench.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._abi import (MipxCfg, MipxImg, MipxInput, MipxOpts, MipxPlan, check, lib, MipxError,
                   EXTEND, GRAVITY, TYPES, OP_YCC, OP_JPEGC, OP_JPEGD, OP_JPEGRT, OP_JPEGE, OP_JPEGH, YCC_444, YCC_420, YCC_422, YCC_GREY,
                   JPEG_SCAN_HEADER_BYTES, JPEG_SCAN_OPT_HEADER_BYTES, JPEGH_OK, JPEGH_UNSYNCED, JPEGH_BAD, sync_tuning)

__all__ = ["DeviceBuffer", "GuardedBuffer", "guard_damage", "set_guard", "guard_setting", "guarded_calls",
           "make_opts", "make_input", "plan_make", "plan_textmark_geometry", "plan_add_textmark",
           "plan_set_ycc_input", "ycc_bytes", "ycc_to_rgb", "YCC_444", "YCC_420", "YCC_422", "YCC_GREY",
           "plan_set_jpegc_output", "jpegc_bytes", "jpeg_qtables", "rgb_to_jpegc",
           "plan_set_jpegd_input", "plan_set_jpegd_input_scaled", "jpegd_bytes", "jpegd_to_rgb", "jpegd_to_rgb_scaled",
           "plan_add_jpeg_roundtrip", "jpeg_roundtrip",
           "plan_set_jpeg_scan_output", "jpeg_scan_bytes", "jpeg_scan_opt_bytes", "rgb_to_jpeg_scan", "jpegc_to_scan", "scan_slot",
           "rgb_to_jpeg_scan_packed", "jpegc_to_scan_packed", "scan_unpack",
           "jpegh_bytes", "plan_set_jpegh_input", "plan_set_jpegh_input_scaled", "execute_status", "jpegh_to_jpegd", "jpegh_to_rgb", "jpegh_to_rgb_scaled", "JPEGH_OK", "JPEGH_UNSYNCED", "JPEGH_BAD",
           "fit_dimension", "Engine",
           "run_op", "execute", "device_count", "synchronize", "set_reduce_sampling", "reduce_sampling"]

SAMPLING = {"corner": 0, "centre": 1}


def set_reduce_sampling(convention: str) -> None:
    """libvips' Lanczos3 reduce sampling convention, PARITY_ASSUMPTIONS.md row 1:
    "corner" (X = o * shrink) or "centre" (X = (o + 0.5) * shrink - 0.5).  Set it
    while no work is in flight (mipx_set_reduce_sampling)."""
    check(lib.mipx_set_reduce_sampling(SAMPLING[convention]), "mipx_set_reduce_sampling")


def reduce_sampling() -> str:
    return {v: k for k, v in SAMPLING.items()}[lib.mipx_reduce_sampling()]


def device_count() -> int:
    return int(lib.mipx_device_count())


def synchronize():
    check(lib.mipx_device_sync(), "mipx_device_sync")


class DeviceBuffer:
    """Raw device allocation owned by Python (freed on close / GC)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(max(nbytes, 1))
        p = C.c_void_p()
        check(lib.mipx_dev_malloc(C.byref(p), self.nbytes), "mipx_dev_malloc")
        self.ptr = p.value

    @classmethod
    def from_array(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = cls(a.nbytes)
        check(lib.mipx_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes), "mipx_memcpy_h2d")
        return b

    def download(self, shape, dtype=np.uint8) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(lib.mipx_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "mipx_memcpy_d2h")
        return out

    def close(self):
        if getattr(self, "ptr", None):
            lib.mipx_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def guard_damage(fill: int, before: np.ndarray, after: np.ndarray, nbytes: int):
    """The pure comparison behind GuardedBuffer.check: `before` / `after` are the guard
    bytes downloaded from in front of and behind a payload of `nbytes`, both expected to
    be all `fill`.  None when they are; otherwise (first, last, count): the first and last
    damaged offsets relative to the payload (before[-1] is offset -1, after[0] is offset
    nbytes) and the number of damaged bytes."""
    before = np.asarray(before, dtype=np.uint8).ravel()
    after = np.asarray(after, dtype=np.uint8).ravel()
    bad = np.concatenate([np.flatnonzero(before != fill) - before.size,
                          np.flatnonzero(after != fill) + int(nbytes)])
    if bad.size == 0:
        return None
    return int(bad[0]), int(bad[-1]), int(bad.size)


class GuardedBuffer:
    """A device payload of `nbytes` between two guard bands, in one allocation of
    G + skew + nbytes + G bytes that starts out all `fill`; the payload begins at
    base + G + skew.  G is a multiple of 4096, so with skew 0 the payload keeps the
    alignment class of a plain allocation: 4096 * ceil((2 * row_bytes + 256) / 4096) for
    an image buffer whose rows are `row_bytes` (w * bands) long, 4096 with row_bytes 0
    (workspaces, the smartcrop origins).  check() finds bytes written into either band.
    G is the detection window: a stray write further than G from the payload is not
    seen (and is not safe either)."""

    @staticmethod
    def guard_bytes(row_bytes: int = 0) -> int:
        return 4096 * -(-(2 * int(row_bytes) + 256) // 4096) if row_bytes else 4096

    def __init__(self, nbytes: int, fill: int, row_bytes: int = 0, skew: int = 0, name: str = "buf",
                 op: str = ""):
        self.nbytes = int(nbytes)
        self.fill = int(fill) & 0xFF
        self.skew = int(skew)
        self.name, self.op = name, op
        self.guard = self.guard_bytes(row_bytes)
        self.total = self.guard + self.skew + self.nbytes + self.guard
        p = C.c_void_p()
        check(lib.mipx_dev_malloc(C.byref(p), self.total), "mipx_dev_malloc")
        self.base = p.value
        self.ptr = self.base + self.guard + self.skew
        check(lib.mipx_memset_dev(self.base, self.fill, self.total), "mipx_memset_dev")

    def upload(self, a: np.ndarray) -> "GuardedBuffer":
        a = np.ascontiguousarray(a, dtype=np.uint8)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        check(lib.mipx_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes), "mipx_memcpy_h2d")
        return self

    def download(self, shape, dtype=np.uint8) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        check(lib.mipx_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "mipx_memcpy_d2h")
        return out

    def damage(self):
        """guard_damage() of both bands as they are now (call after the synchronise)."""
        before = np.empty(self.guard + self.skew, np.uint8)
        after = np.empty(self.guard, np.uint8)
        check(lib.mipx_memcpy_d2h(before.ctypes.data, self.base, before.nbytes), "mipx_memcpy_d2h")
        check(lib.mipx_memcpy_d2h(after.ctypes.data, self.ptr + self.nbytes, after.nbytes), "mipx_memcpy_d2h")
        return guard_damage(self.fill, before, after, self.nbytes)

    def check(self, what: str = "") -> None:
        d = self.damage()
        if d is not None:
            first, last, count = d
            raise AssertionError(
                f"{what or self.op}: guard of buffer '{self.name}' damaged: {count} byte(s), first at payload "
                f"offset {first}, last at {last} (payload 0..{self.nbytes - 1}, fill 0x{self.fill:02X}, "
                f"skew {self.skew})")

    def close(self):
        if getattr(self, "base", None):
            lib.mipx_dev_free(self.base)
            self.base = self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# (fill, skew_in, skew_out) while run_op / smartcrop_origins / execute guard their buffers; None = off
_guard = None
_guarded_calls = 0


def set_guard(fill: Optional[int] = None, skew_in: int = 0, skew_out: int = 0):
    """Footprint checking for run_op, smartcrop_origins and execute (tests; off by
    default).  With a fill byte, every device buffer of a call (in / out / wm / ws /
    origins) is a GuardedBuffer: output and workspace start as `fill`, the workspace is
    exactly the advertised size, the input (skew_in) and output (skew_out) payloads start
    that many bytes off the allocation's alignment, and every guard is checked before
    the result is returned.  Returns the previous setting, which set_guard(*prev)
    restores."""
    global _guard
    prev = _guard if _guard is not None else (None, 0, 0)
    _guard = None if fill is None else (int(fill) & 0xFF, int(skew_in), int(skew_out))
    return prev


def guard_setting():
    return _guard


def guarded_calls() -> int:
    """How many run_op / smartcrop_origins / execute calls have checked their guards."""
    return _guarded_calls


def _dev(name: str, op: str, nbytes: int, row_bytes: int = 0, data: Optional[np.ndarray] = None):
    """One device buffer of a call: a plain DeviceBuffer, or a GuardedBuffer while
    set_guard is on."""
    if _guard is None:
        return DeviceBuffer.from_array(data) if data is not None else DeviceBuffer(nbytes)
    fill, skew_in, skew_out = _guard
    skew = skew_in if name == "in" else skew_out if name == "out" else 0
    b = GuardedBuffer(data.nbytes if data is not None else nbytes, fill, row_bytes, skew, name, op)
    return b.upload(data) if data is not None else b


def _check_guards(op: str, *bufs) -> None:
    global _guarded_calls
    if _guard is None:
        return
    for b in bufs:
        if b is not None:
            b.check(op)
    _guarded_calls += 1


def make_opts(**kw) -> MipxOpts:
    """MipxOpts from bimg-style keyword fields (see include/mipx.h)."""
    o = MipxOpts()
    for k, v in kw.items():
        if k == "background":
            o.background[:] = list(v)[:3]
        elif k == "gravity" and isinstance(v, str):
            o.gravity = GRAVITY[v]
        elif k == "extend" and isinstance(v, str):
            o.extend = EXTEND[v]
        else:
            setattr(o, k, v)
    return o


def make_input(w, h, bands, type="unknown", orientation=0, decoded_w=0, decoded_h=0,
               wm_w=0, wm_h=0, wm_bands=0) -> MipxInput:
    i = MipxInput()
    i.w, i.h, i.bands = w, h, bands
    i.type = TYPES[type] if isinstance(type, str) else int(type)
    i.orientation = orientation
    i.decoded_w, i.decoded_h = decoded_w, decoded_h
    i.wm_w, i.wm_h, i.wm_bands = wm_w, wm_h, wm_bands
    return i


def plan_make(opts: MipxOpts, inp: MipxInput) -> MipxPlan:
    p = MipxPlan()
    check(lib.mipx_plan_make(C.byref(opts), C.byref(inp), C.byref(p)), "mipx_plan_make")
    return p


def plan_chain(stages) -> MipxPlan:
    """mipx_plan_chain: one plan for a /pipeline chain of stage plans."""
    arr = (MipxPlan * len(stages))(*stages)
    p = MipxPlan()
    check(lib.mipx_plan_chain(arr, len(stages), C.byref(p)), "mipx_plan_chain")
    return p


def plan_textmark_geometry(plan: MipxPlan):
    """mipx_plan_textmark_geometry: (w, h, bands) of the image where a text watermark
    step would go (after the blur, before the watermark image, flatten and B_W)."""
    w, h, b = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.mipx_plan_textmark_geometry(C.byref(plan), C.byref(w), C.byref(h), C.byref(b)),
          "mipx_plan_textmark_geometry")
    return w.value, h.value, b.value


def plan_add_textmark(plan: MipxPlan, mask_w: int, mask_h: int, margin: int, opacity: float,
                      colour=(0, 0, 0), no_replicate: bool = False) -> MipxPlan:
    """mipx_plan_add_textmark on `plan` (in place; returned for convenience): the rendered
    text mask then travels as the request's watermark image."""
    check(lib.mipx_plan_add_textmark(C.byref(plan), mask_w, mask_h, margin, opacity,
                                     (C.c_int32 * 3)(*list(colour)[:3]), int(bool(no_replicate))),
          "mipx_plan_add_textmark")
    return plan


def ycc_bytes(w: int, h: int, layout: int) -> int:
    """mipx_ycc_bytes: bytes of one image's packed planes (0 for bad arguments)."""
    return int(lib.mipx_ycc_bytes(w, h, layout))


def plan_set_ycc_input(plan: MipxPlan, layout: int) -> MipxPlan:
    """mipx_plan_set_ycc_input on `plan` (in place; returned for convenience): the plan then
    takes packed JPEG planes (Y, Cb, Cr; YCC_444, YCC_420 or YCC_422) instead of RGB pixels."""
    check(lib.mipx_plan_set_ycc_input(C.byref(plan), layout), "mipx_plan_set_ycc_input")
    return plan


def _ycc_layout(plan: MipxPlan):
    """The plane layout a plan's input has, or None for interleaved pixels."""
    return plan.steps[0].a[0] if plan.n_steps > 0 and plan.steps[0].op == OP_YCC else None


def _jpegd_layout(plan: MipxPlan):
    """The layout of the coefficient payload a plan's input is, or None for anything else."""
    return plan.steps[0].a[0] if plan.n_steps > 0 and plan.steps[0].op == OP_JPEGD else None


def _jpegd_file_size(plan: MipxPlan):
    """(w, h) of the file whose payload a JPEGD plan takes: the plan's input size, or what a
    scaled step (a[1] = 2, 4, 8) carries in a[2], a[3]."""
    a = plan.steps[0].a
    return (a[2], a[3]) if a[1] > 1 else (plan.in_w, plan.in_h)


def _jpegh_layout(plan: MipxPlan):
    """The layout of the entropy-coded slot a plan's input is, or None for anything else."""
    return plan.steps[0].a[0] if plan.n_steps > 0 and plan.steps[0].op == OP_JPEGH else None


def _packed_input(plan: MipxPlan) -> bool:
    """Whether the plan's input is bytes per image (planes, a coefficient payload or a scan's slot), not pixels."""
    return _ycc_layout(plan) is not None or _jpegd_layout(plan) is not None or _jpegh_layout(plan) is not None


def _planes(plan: MipxPlan, planes) -> np.ndarray:
    """A YCC or JPEGD plan's input as (n, bytes) uint8, from (bytes,) or (n, bytes)."""
    x = np.ascontiguousarray(planes, dtype=np.uint8)
    if x.ndim == 1:
        x = x[None]
    if _jpegd_layout(plan) is not None:
        need, what = jpegd_bytes(*_jpegd_file_size(plan), _jpegd_layout(plan)), "coefficient"
    elif _jpegh_layout(plan) is not None:
        need, what = jpegh_bytes(*_jpegd_file_size(plan), _jpegh_layout(plan)), "scan"
    else:
        need, what = ycc_bytes(plan.in_w, plan.in_h, _ycc_layout(plan)), "planar"
    if x.ndim != 2 or x.shape[1] != need:
        raise ValueError(f"{what} input of shape {np.shape(planes)}: the plan takes ({need},) or (n, {need}) uint8")
    return x


def jpegd_bytes(w: int, h: int, layout: int) -> int:
    """mipx_jpegd_bytes: bytes of one image's coefficient payload, the 384 bytes of quantisation
    tables and jpegc_bytes of coefficients (0 for bad arguments)."""
    return int(lib.mipx_jpegd_bytes(w, h, layout))


def plan_set_jpegd_input(plan: MipxPlan, layout: int) -> MipxPlan:
    """mipx_plan_set_jpegd_input on `plan` (in place; returned for convenience): the plan then
    takes a JPEG's quantisation tables and quantised coefficients (codec.decode_jpeg_coefs;
    YCC_444, YCC_420 or YCC_422) instead of RGB pixels; a 1-band plan takes YCC_GREY."""
    check(lib.mipx_plan_set_jpegd_input(C.byref(plan), layout), "mipx_plan_set_jpegd_input")
    return plan


def plan_set_jpegd_input_scaled(plan: MipxPlan, layout: int, shrink: int, file_w: int, file_h: int) -> MipxPlan:
    """mipx_plan_set_jpegd_input_scaled on `plan` (in place; returned for convenience): the plan,
    made for the ceil(file_w / shrink) x ceil(file_h / shrink) decode, then takes the full-size
    file's coefficient payload and decodes it at 1/shrink (1, 2, 4, 8) as libjpeg's
    shrink-on-load does.  shrink 1 is plan_set_jpegd_input."""
    check(lib.mipx_plan_set_jpegd_input_scaled(C.byref(plan), layout, shrink, file_w, file_h),
          "mipx_plan_set_jpegd_input_scaled")
    return plan


def plan_set_jpegh_input(plan: MipxPlan, layout: int) -> MipxPlan:
    """mipx_plan_set_jpegh_input on `plan` (in place; returned for convenience): the plan then
    takes a JPEG's tables and entropy-coded scan (codec.jpeg_huff_slot; YCC_444, YCC_420 or YCC_422)
    instead of RGB pixels."""
    check(lib.mipx_plan_set_jpegh_input(C.byref(plan), layout), "mipx_plan_set_jpegh_input")
    return plan


def plan_set_jpegh_input_scaled(plan: MipxPlan, layout: int, shrink: int, file_w: int, file_h: int) -> MipxPlan:
    """mipx_plan_set_jpegh_input_scaled: as plan_set_jpegd_input_scaled, on the file's slot."""
    check(lib.mipx_plan_set_jpegh_input_scaled(C.byref(plan), layout, shrink, file_w, file_h),
          "mipx_plan_set_jpegh_input_scaled")
    return plan


def jpegc_bytes(w: int, h: int, layout: int) -> int:
    """mipx_jpegc_bytes: bytes of one image's JPEG coefficients (0 for bad arguments)."""
    return int(lib.mipx_jpegc_bytes(w, h, layout))


def jpeg_qtables(quality: int):
    """mipx_jpeg_qtables: (lum, chr), 64 uint8 each in natural order, of jpeg_set_quality."""
    lum, chrom = np.empty(64, np.uint8), np.empty(64, np.uint8)
    check(lib.mipx_jpeg_qtables(quality, lum.ctypes.data_as(C.POINTER(C.c_uint8)),
                                chrom.ctypes.data_as(C.POINTER(C.c_uint8))), "mipx_jpeg_qtables")
    return lum, chrom


def plan_set_jpegc_output(plan: MipxPlan, layout: int, quality: int) -> MipxPlan:
    """mipx_plan_set_jpegc_output on `plan` (in place; returned for convenience): the plan then
    gives the quantised DCT coefficients of its 3-band result (YCC_444 or YCC_420; YCC_GREY of a 1-band one; made at
    `quality`) instead of RGB pixels."""
    check(lib.mipx_plan_set_jpegc_output(C.byref(plan), layout, quality), "mipx_plan_set_jpegc_output")
    return plan


def plan_add_jpeg_roundtrip(plan: MipxPlan, layout: int, quality: int, shrink: int = 1) -> MipxPlan:
    """mipx_plan_add_jpeg_roundtrip on `plan` (in place; returned for convenience): the plan's
    3-band result then goes through a JPEG of itself (YCC_444 or YCC_420, made at `quality`)
    decoded at 1/shrink (1, 2, 4, 8), as a re-encode and decode on the host would leave it; more
    steps, a text watermark and plan_set_jpegc_output may follow."""
    check(lib.mipx_plan_add_jpeg_roundtrip(C.byref(plan), layout, quality, shrink), "mipx_plan_add_jpeg_roundtrip")
    return plan


def _jpegc_layout(plan: MipxPlan):
    """The layout of the coefficients a plan gives, or None for interleaved pixels."""
    last = plan.steps[plan.n_steps - 1] if plan.n_steps > 0 else None
    return last.a[0] if last is not None and last.op == OP_JPEGC else None


def jpeg_scan_bytes(w: int, h: int, layout: int) -> int:
    """mipx_jpeg_scan_bytes: bytes of one image's entropy-coded output slot (0 for bad arguments)."""
    return int(lib.mipx_jpeg_scan_bytes(w, h, layout))


def jpeg_scan_opt_bytes(w: int, h: int, layout: int) -> int:
    """mipx_jpeg_scan_opt_bytes: bytes of one image's output slot with optimised Huffman tables."""
    return int(lib.mipx_jpeg_scan_opt_bytes(w, h, layout))


def plan_set_jpeg_scan_output(plan: MipxPlan, layout: int, quality: int, optimize: bool = False) -> MipxPlan:
    """mipx_plan_set_jpeg_scan_output on `plan` (in place; returned for convenience): the plan then
    gives the finished entropy-coded scan of its 3-band result (YCC_444 or YCC_420; YCC_GREY of a 1-band one; made at
    `quality`), one slot per image (scan_slot reads it), instead of RGB pixels.  optimize: coded with
    the image's own Huffman tables, which the slot then carries (mipx_plan_set_jpeg_scan_output_optimized)."""
    if optimize:
        check(lib.mipx_plan_set_jpeg_scan_output_optimized(C.byref(plan), layout, quality),
              "mipx_plan_set_jpeg_scan_output_optimized")
    else:
        check(lib.mipx_plan_set_jpeg_scan_output(C.byref(plan), layout, quality), "mipx_plan_set_jpeg_scan_output")
    return plan


def _jpege_layout(plan: MipxPlan):
    """The layout of the scan a plan gives, or None for anything else."""
    last = plan.steps[plan.n_steps - 1] if plan.n_steps > 0 else None
    return last.a[0] if last is not None and last.op == OP_JPEGE else None


def _jpege_slot_bytes(plan: MipxPlan):
    """Bytes of one output slot of a plan that gives scans, with or without its tables."""
    last = plan.steps[plan.n_steps - 1]
    return (jpeg_scan_opt_bytes if last.a[2] else jpeg_scan_bytes)(plan.out_w, plan.out_h, last.a[0])


def scan_slot(slot, tables: bool = False):
    """(status, bits, scan) of one output slot of MIPX_OP_JPEGE (uint8, jpeg_scan_bytes long):
    scan is the `length` bytes behind the header, empty unless status is 0 (codec.jpeg_from_scan
    makes the file of it).  With `tables`, (status, bits, scan, tables): for a slot with optimised
    Huffman tables (jpeg_scan_opt_bytes long; the header's last word says which it is) the four it
    carries as codec.jpeg_header takes them, by DHT Tc/Th byte; None for an Annex K slot or a
    status other than 0."""
    slot = np.ascontiguousarray(slot, dtype=np.uint8).ravel()
    length, status, bits, kind = (int(v) for v in slot[:JPEG_SCAN_HEADER_BYTES].view("<u4"))
    head = JPEG_SCAN_OPT_HEADER_BYTES if kind == 1 else JPEG_SCAN_HEADER_BYTES
    if status != 0:
        return (status, bits, b"", None) if tables else (status, bits, b"")
    if slot.size < head or length > slot.size - head:
        raise ValueError(f"slot of {slot.size} bytes says its scan has {length}")
    scan = slot[head:head + length].tobytes()
    if not tables:
        return status, bits, scan
    found = None
    if kind == 1:
        found = {}
        for k, tc in enumerate((0x00, 0x01, 0x10, 0x11)):   # DC 0, DC 1, AC 0, AC 1
            t = slot[JPEG_SCAN_HEADER_BYTES + 272 * k:JPEG_SCAN_HEADER_BYTES + 272 * (k + 1)]
            found[tc] = (t[:16].tobytes(), t[16:16 + int(t[:16].sum())].tobytes())
    return status, bits, scan, found


def fit_dimension(iw, ih, fw, fh):
    a, b = C.c_int32(), C.c_int32()
    check(lib.mipx_fit_dimension(iw, ih, fw, fh, C.byref(a), C.byref(b)), "mipx_fit_dimension")
    return a.value, b.value


def _img(a: np.ndarray) -> MipxImg:
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, b = a.shape
    m = MipxImg(a.ctypes.data, w, h, b, a.strides[0])
    return m


class Engine:
    """Request path: pinned staging, per-device queues, batching (mipx_submit/mipx_wait)."""

    def __init__(self, devices: Optional[Sequence[int]] = None, max_batch: int = 64,
                 batch_wait_us: int = 0, queues_per_device: int = 1):
        cfg = MipxCfg()
        cfg.queues_per_device = queues_per_device
        if devices:
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices):
                cfg.device_ids[i] = d
        cfg.max_batch = max_batch
        cfg.batch_wait_us = batch_wait_us
        sync_tuning()
        check(lib.mipx_init(C.byref(cfg)), "mipx_init")

    @classmethod
    def attach(cls) -> "Engine":
        """A handle on the engine already running in this process (started by another
        Engine, with whatever configuration it chose); mipx_init is not called."""
        if lib.mipx_queue_count() <= 0:
            raise MipxError(-7, "Engine.attach: no engine running")
        return cls.__new__(cls)

    def submit(self, plan: MipxPlan, img: np.ndarray, wm: Optional[np.ndarray] = None, device: int = -1,
               out: Optional[np.ndarray] = None):
        """Queue one request; returns (ticket, out).  `out` (optional) receives the
        result: contiguous uint8 of the plan's output shape.  The MIPX_* kernel knobs are
        re-read in Engine(), run_op and execute, not per request: a reload
        must not race the queue workers' launches."""
        planar = _packed_input(plan)
        if planar:  # the packed planes or the payload of one image, described as the plan's w x h x bands
            img = _planes(plan, img)
            if img.shape[0] != 1:
                raise ValueError("submit takes one image's planes or payload")
        elif not (img.dtype == np.uint8 and img.ndim == 3 and img.strides[2] == 1
                  and img.strides[1] == img.shape[2]):
            img = np.ascontiguousarray(img, dtype=np.uint8)  # rows may keep a wider stride
        coefs = _jpegc_layout(plan)
        scan = _jpege_layout(plan)
        if coefs is not None:  # the coefficients of one image, described as the plan's w x h x bands
            shape, dtype = (jpegc_bytes(plan.out_w, plan.out_h, coefs) // 2,), np.int16
        elif scan is not None:  # ... or its slot
            shape, dtype = (_jpege_slot_bytes(plan),), np.uint8
        else:
            shape, dtype = (plan.out_h, plan.out_w, plan.out_bands), np.uint8
        if out is None:
            out = np.empty(shape, dtype)
        elif out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"out must be contiguous {np.dtype(dtype).name} {shape}")
        ti = C.c_uint64()
        wm = np.ascontiguousarray(wm, dtype=np.uint8) if wm is not None else None  # a copy must live until the submit
        wmi = C.byref(_img(wm)) if wm is not None else None
        src = MipxImg(img.ctypes.data, plan.in_w, plan.in_h, plan.in_bands, 0) if planar else _img(img)
        packed = coefs is not None or scan is not None
        dst = MipxImg(out.ctypes.data, plan.out_w, plan.out_h, plan.out_bands, 0) if packed else _img(out)
        check(lib.mipx_submit(device, C.byref(plan), C.byref(src), wmi, C.byref(dst),
                              C.byref(ti)), "mipx_submit")
        return ti.value, out

    def wait(self, ticket: int, timeout_ms: int = -1):
        check(lib.mipx_wait(ticket, timeout_ms), "mipx_wait")

    def process(self, plan: MipxPlan, img: np.ndarray, wm: Optional[np.ndarray] = None) -> np.ndarray:
        t, out = self.submit(plan, img, wm)
        self.wait(t)
        return out

    def stats(self, device: int = 0):
        """(batches launched, requests retired) on `device` since mipx_init."""
        b, r = C.c_uint64(), C.c_uint64()
        check(lib.mipx_stats(device, C.byref(b), C.byref(r)), "mipx_stats")
        return b.value, r.value

    def transfer_stats(self, queue: int = 0):
        """(H2D bytes, D2H bytes) the request path has enqueued on `queue` since mipx_init."""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib.mipx_transfer_stats(queue, C.byref(a), C.byref(b)), "mipx_transfer_stats")
        return a.value, b.value

    def queue_stats(self):
        """[(device, batches, requests, pending_bytes)] for every request queue."""
        out = []
        for q in range(lib.mipx_queue_count()):
            d, b, r, p = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_int64()
            check(lib.mipx_queue_stats(q, C.byref(d), C.byref(b), C.byref(r), C.byref(p)), "mipx_queue_stats")
            out.append((d.value, b.value, r.value, p.value))
        return out

    def cancel(self, ticket: int):
        check(lib.mipx_cancel(ticket), "mipx_cancel")

    def shutdown(self):
        lib.mipx_shutdown()


def _batch(imgs) -> np.ndarray:
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim == 3:
        a = a[None]
    return a


def run_op(name: str, imgs: np.ndarray, **p) -> np.ndarray:
    """Run one mipx_op_* kernel on a batch (n, h, w, b) of host images; returns host output."""
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    what = f"mipx_op_{name}"
    din = _dev("in", what, x.nbytes, w * b, x)
    ws = None
    dwm = None
    wsb = 0
    if name == "reduce":
        hs, vs = p["hshrink"], p["vshrink"]
        oh, ow, ob = _osz_reduce(h, vs), _osz_reduce(w, hs), b
        wsb = lib.mipx_op_workspace_bytes(4, n, w, h, b, hs, vs)
    elif name == "reducev":
        oh, ow, ob = _osz_reduce(h, p["vshrink"]), w, b
    elif name == "reduceh":
        oh, ow, ob = h, _osz_reduce(w, p["hshrink"]), b
    elif name == "shrink":
        oh, ow, ob = _osz_shrink(h, p["vshrink"]), _osz_shrink(w, p["hshrink"]), b
    elif name == "embed":
        oh, ow, ob = p["height"], p["width"], b
    elif name == "extract":
        oh, ow, ob = p["height"], p["width"], b
    elif name == "rot":
        a = p["angle"] % 360
        oh, ow, ob = (w, h, b) if a in (90, 270) else (h, w, b)
    elif name == "flip":
        oh, ow, ob = h, w, b
    elif name == "gaussblur":
        oh, ow, ob = h, w, b
        wsb = lib.mipx_op_workspace_bytes(8, n, w, h, b, p["sigma"], p.get("min_ampl", 0.2))
    elif name == "watermark":
        oh, ow = h, w
        ob = b if b in (2, 4) else b + 1
    elif name == "textmark":
        oh, ow, ob = h, w, 3
    elif name == "affine":
        import math
        ow, oh, ob = int(math.ceil(w * p["xscale"])), int(math.ceil(h * p["yscale"])), b
    elif name == "zoom":
        ow, oh, ob = w * p["xfac"], h * p["yfac"], b
    elif name == "flatten":
        oh, ow, ob = h, w, (b - 1 if b in (2, 4) else b)
    elif name == "bw":
        oh, ow, ob = h, w, (2 if b == 4 else 1 if b == 3 else b)
    else:
        raise ValueError(name)
    dout = _dev("out", what, n * oh * ow * ob, ow * ob)
    if wsb:
        ws = _dev("ws", what, wsb)
    wsp = ws.ptr if ws else None
    if name == "reduce":
        code = lib.mipx_op_reduce(din.ptr, dout.ptr, n, w, h, b, hs, vs, wsp, wsb, None)
    elif name == "reducev":
        code = lib.mipx_op_reducev(din.ptr, dout.ptr, n, w, h, b, p["vshrink"], None)
    elif name == "reduceh":
        code = lib.mipx_op_reduceh(din.ptr, dout.ptr, n, w, h, b, p["hshrink"], None)
    elif name == "shrink":
        code = lib.mipx_op_shrink(din.ptr, dout.ptr, n, w, h, b, p["hshrink"], p["vshrink"], None)
    elif name == "embed":
        bg = (C.c_int32 * 3)(*p.get("background", (0, 0, 0)))
        code = lib.mipx_op_embed(din.ptr, dout.ptr, n, w, h, b, p["x"], p["y"], p["width"], p["height"],
                                 p["extend"], bg, None)
    elif name == "extract":
        code = lib.mipx_op_extract(din.ptr, dout.ptr, n, w, h, b, p["left"], p["top"], p["width"],
                                   p["height"], None)
    elif name == "rot":
        code = lib.mipx_op_rot(din.ptr, dout.ptr, n, w, h, b, p["angle"], None)
    elif name == "flip":
        code = lib.mipx_op_flip(din.ptr, dout.ptr, n, w, h, b, int(p["vertical"]), None)
    elif name == "gaussblur":
        code = lib.mipx_op_gaussblur(din.ptr, dout.ptr, n, w, h, b, p["sigma"], p.get("min_ampl", 0.2),
                                     wsp, wsb, None)
    elif name == "watermark":
        wm = np.ascontiguousarray(p["wm"], dtype=np.uint8)
        if wm.ndim == 2:
            wm = wm[:, :, None]
        dwm = _dev("wm", what, wm.nbytes, wm.shape[1] * wm.shape[2], wm)
        code = lib.mipx_op_watermark(din.ptr, dwm.ptr, dout.ptr, n, w, h, b, wm.shape[1], wm.shape[0],
                                     wm.shape[2], p["left"], p["top"], p["opacity"], None)
    elif name == "textmark":
        mask = np.ascontiguousarray(p["mask"], dtype=np.uint8)
        dwm = _dev("wm", what, mask.nbytes, mask.shape[1], mask)
        code = lib.mipx_op_text_watermark(din.ptr, dwm.ptr, dout.ptr, n, w, h, b, mask.shape[1], mask.shape[0],
                                          p["margin"], p["opacity"], (C.c_int32 * 3)(*p["colour"]), None)
    elif name == "affine":
        code = lib.mipx_op_affine(din.ptr, dout.ptr, n, w, h, b, p["xscale"], p["yscale"], p.get("extend", 1), None)
    elif name == "zoom":
        code = lib.mipx_op_zoom(din.ptr, dout.ptr, n, w, h, b, p["xfac"], p["yfac"], None)
    elif name == "flatten":
        code = lib.mipx_op_flatten(din.ptr, dout.ptr, n, w, h, b, (C.c_int32 * 3)(*p["background"]), None)
    elif name == "bw":
        code = lib.mipx_op_colourspace_bw(din.ptr, dout.ptr, n, w, h, b, None)
    check(code, what)
    synchronize()
    _check_guards(what, din, dout, dwm, ws)
    return dout.download((n, oh, ow, ob))


def ycc_to_rgb(planes: np.ndarray, w: int, h: int, layout: int) -> np.ndarray:
    """mipx_op_ycc_to_rgb on packed planes, (bytes,) or (n, bytes) uint8; returns (n, h, w, 3)."""
    sync_tuning()
    x = np.ascontiguousarray(planes, dtype=np.uint8)
    if x.ndim == 1:
        x = x[None]
    need = ycc_bytes(w, h, layout)
    if x.ndim != 2 or need == 0 or x.shape[1] != need:
        raise ValueError(f"planes of shape {np.shape(planes)} for {w}x{h} layout {layout}: {need} bytes per image")
    n = x.shape[0]
    what = "mipx_op_ycc_to_rgb"
    din = _dev("in", what, x.nbytes, w, x)
    dout = _dev("out", what, n * h * w * 3, w * 3)
    check(lib.mipx_op_ycc_to_rgb(din.ptr, dout.ptr, n, w, h, layout, None), what)
    synchronize()
    _check_guards(what, din, dout)
    return dout.download((n, h, w, 3))


def rgb_to_jpegc(imgs: np.ndarray, layout: int, quality: int) -> np.ndarray:
    """mipx_op_rgb_to_jpegc on (h, w, 3) or (n, h, w, 3) uint8; returns the coefficients,
    (n, jpegc_bytes / 2) int16.  With YCC_GREY the images are (n, h, w, 1)."""
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    need = jpegc_bytes(w, h, layout)
    if b != (1 if layout == YCC_GREY else 3) or need == 0:
        raise ValueError(f"images of shape {np.shape(imgs)}, layout {layout}: RGB and YCC_444 / YCC_420, "
                         "or 1 band and YCC_GREY")
    what = "mipx_op_rgb_to_jpegc"
    din = _dev("in", what, x.nbytes, w * b, x)
    dout = _dev("out", what, n * need, 128 * ((w + 7) // 8))
    check(lib.mipx_op_rgb_to_jpegc(din.ptr, dout.ptr, n, w, h, layout, quality, None), what)
    synchronize()
    _check_guards(what, din, dout)
    return dout.download((n, need // 2), np.int16)


def rgb_to_jpeg_scan(imgs: np.ndarray, layout: int, quality: int, optimize: bool = False) -> np.ndarray:
    """mipx_op_rgb_to_jpeg_scan on (h, w, 3) or (n, h, w, 3) uint8; returns the slots,
    (n, jpeg_scan_bytes) uint8; with `optimize` mipx_op_rgb_to_jpeg_scan_optimized and
    (n, jpeg_scan_opt_bytes)."""
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    need = (jpeg_scan_opt_bytes if optimize else jpeg_scan_bytes)(w, h, layout)
    if b != (1 if layout == YCC_GREY else 3) or need == 0:
        raise ValueError(f"images of shape {np.shape(imgs)}, layout {layout}: RGB and YCC_444 / YCC_420, "
                         "or 1 band and YCC_GREY")
    what = "mipx_op_rgb_to_jpeg_scan_optimized" if optimize else "mipx_op_rgb_to_jpeg_scan"
    din = _dev("in", what, x.nbytes, w * b, x)
    dout = _dev("out", what, n * need, 128 * ((w + 7) // 8))
    ws = _dev("ws", what, lib.mipx_op_workspace_bytes(OP_JPEGE, n, w, h, 3, 1.0 if optimize else 0.0, 0.0))
    check(getattr(lib, what)(din.ptr, dout.ptr, n, w, h, layout, quality, ws.ptr, None), what)
    synchronize()
    _check_guards(what, din, dout, ws)
    return dout.download((n, need))


def jpegc_to_scan(coefs: np.ndarray, w: int, h: int, layout: int, optimize: bool = False) -> np.ndarray:
    """mipx_op_jpegc_to_scan on coefficients as rgb_to_jpegc returns them, (jpegc_bytes / 2,) or
    (n, jpegc_bytes / 2) int16; returns the slots, (n, jpeg_scan_bytes) uint8; with `optimize`
    mipx_op_jpegc_to_scan_optimized and (n, jpeg_scan_opt_bytes)."""
    sync_tuning()
    x = np.ascontiguousarray(coefs, dtype=np.int16)
    if x.ndim == 1:
        x = x[None]
    have = jpegc_bytes(w, h, layout)
    if x.ndim != 2 or have == 0 or x.shape[1] * 2 != have:
        raise ValueError(f"coefficients of shape {np.shape(coefs)} for {w}x{h} layout {layout}: {have // 2} per image")
    n, need = x.shape[0], (jpeg_scan_opt_bytes if optimize else jpeg_scan_bytes)(w, h, layout)
    what = "mipx_op_jpegc_to_scan_optimized" if optimize else "mipx_op_jpegc_to_scan"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x.view(np.uint8))
    dout = _dev("out", what, n * need, 128 * ((w + 7) // 8))
    ws = _dev("ws", what, lib.mipx_op_workspace_bytes(OP_JPEGE, n, w, h, 3, 1.0 if optimize else 0.0, 0.0))
    check(getattr(lib, what)(din.ptr, dout.ptr, n, w, h, layout, ws.ptr, None), what)
    synchronize()
    _check_guards(what, din, dout, ws)
    return dout.download((n, need))


def _packed_result(what: str, n: int, need: int, call, w: int, din, ws):
    """The output side the two packed calls share: the slots' buffer, the workspace and the directory
    (behind 8 spare bytes, so that the output skew keeps it 8-byte aligned), the call, (dir, packed)."""
    dout = _dev("out", what, n * need, 128 * ((w + 7) // 8))
    ddir = _dev("out", what, 8 * (n + 1) + 8)
    at = ddir.ptr + (-ddir.ptr) % 8
    check(call(dout, at), what)
    synchronize()
    _check_guards(what, din, dout, ddir, ws)
    d = np.empty(n + 1, "<u8")
    check(lib.mipx_memcpy_d2h(d.ctypes.data, at, d.nbytes), "mipx_memcpy_d2h")
    return d, dout.download((n * need,))


def rgb_to_jpeg_scan_packed(imgs: np.ndarray, layout: int, quality: int, optimize: bool = False):
    """mipx_op_rgb_to_jpeg_scan_packed on (h, w, 3) or (n, h, w, 3) uint8; returns (dir, packed): the n + 1
    uint64 offsets and the whole output buffer, n * jpeg_scan_bytes (jpeg_scan_opt_bytes with `optimize`)
    uint8, of which only each slot's header and scan were written (scan_unpack takes one slot out)."""
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    need = (jpeg_scan_opt_bytes if optimize else jpeg_scan_bytes)(w, h, layout)
    if b != (1 if layout == YCC_GREY else 3) or need == 0:
        raise ValueError(f"images of shape {np.shape(imgs)}, layout {layout}: RGB and YCC_444 / YCC_420, "
                         "or 1 band and YCC_GREY")
    what = "mipx_op_rgb_to_jpeg_scan_packed"
    din = _dev("in", what, x.nbytes, w * b, x)
    ws = _dev("ws", what, lib.mipx_op_workspace_bytes(OP_JPEGE, n, w, h, 3, 1.0 if optimize else 0.0, 0.0))
    out = _packed_result(what, n, need, lambda dout, ddir: lib.mipx_op_rgb_to_jpeg_scan_packed(
        din.ptr, dout.ptr, n, w, h, layout, quality, ws.ptr, None, int(bool(optimize)), ddir), w, din, ws)
    return out


def jpegc_to_scan_packed(coefs: np.ndarray, w: int, h: int, layout: int, optimize: bool = False):
    """mipx_op_jpegc_to_scan_packed on coefficients as rgb_to_jpegc returns them; returns (dir, packed) as
    rgb_to_jpeg_scan_packed does."""
    sync_tuning()
    x = np.ascontiguousarray(coefs, dtype=np.int16)
    if x.ndim == 1:
        x = x[None]
    have = jpegc_bytes(w, h, layout)
    if x.ndim != 2 or have == 0 or x.shape[1] * 2 != have:
        raise ValueError(f"coefficients of shape {np.shape(coefs)} for {w}x{h} layout {layout}: {have // 2} per image")
    n, need = x.shape[0], (jpeg_scan_opt_bytes if optimize else jpeg_scan_bytes)(w, h, layout)
    what = "mipx_op_jpegc_to_scan_packed"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x.view(np.uint8))
    ws = _dev("ws", what, lib.mipx_op_workspace_bytes(OP_JPEGE, n, w, h, 3, 1.0 if optimize else 0.0, 0.0))
    out = _packed_result(what, n, need, lambda dout, ddir: lib.mipx_op_jpegc_to_scan_packed(
        din.ptr, dout.ptr, n, w, h, layout, ws.ptr, None, int(bool(optimize)), ddir), w, din, ws)
    return out


def scan_unpack(dir, packed, i: int, head: int, slot_bytes: int) -> np.ndarray:
    """mipx_jpeg_scan_unpack: slot i of packed slots as a buffer of slot_bytes uint8 that starts out 0xA5
    and holds the slot's header (`head` bytes: 16, or 1104 with optimised tables) and its scan; MipxError
    (MIPX_EDATA) for a directory or a header that is inconsistent.  Runs on the host, without a GPU."""
    d = np.ascontiguousarray(dir, dtype="<u8")
    p = np.ascontiguousarray(packed, dtype=np.uint8).ravel()
    slot = np.full(int(slot_bytes), 0xA5, np.uint8)
    check(lib.mipx_jpeg_scan_unpack(d.ctypes.data, d.size - 1, p.ctypes.data, p.size, i, head, slot.ctypes.data,
                                    slot.size), "mipx_jpeg_scan_unpack")
    return slot


def jpegd_to_rgb(payload: np.ndarray, w: int, h: int, layout: int) -> np.ndarray:
    """mipx_op_jpegd_to_rgb on coefficient payloads, (bytes,) or (n, bytes) uint8; returns (n, h, w, 3),
    with YCC_GREY (n, h, w, 1)."""
    sync_tuning()
    x = np.ascontiguousarray(payload, dtype=np.uint8)
    if x.ndim == 1:
        x = x[None]
    need = jpegd_bytes(w, h, layout)
    if x.ndim != 2 or need == 0 or x.shape[1] != need:
        raise ValueError(f"payload of shape {np.shape(payload)} for {w}x{h} layout {layout}: {need} bytes per image")
    n = x.shape[0]
    what = "mipx_op_jpegd_to_rgb"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x)
    b = 1 if layout == YCC_GREY else 3
    dout = _dev("out", what, n * h * w * b, w * b)
    wsb = lib.mipx_op_workspace_bytes(OP_JPEGD, n, w, h, 3, 0.0, 0.0)
    ws = _dev("ws", what, wsb)
    check(lib.mipx_op_jpegd_to_rgb(din.ptr, dout.ptr, n, w, h, layout, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, ws)
    return dout.download((n, h, w, b))


def jpegd_to_rgb_scaled(payload: np.ndarray, w: int, h: int, layout: int, shrink: int) -> np.ndarray:
    """mipx_op_jpegd_to_rgb_scaled on the coefficient payloads of w x h files, (bytes,) or
    (n, bytes) uint8; returns (n, ceil(h / shrink), ceil(w / shrink), 3), with YCC_GREY 1 band."""
    sync_tuning()
    x = np.ascontiguousarray(payload, dtype=np.uint8)
    if x.ndim == 1:
        x = x[None]
    need = jpegd_bytes(w, h, layout)
    if x.ndim != 2 or need == 0 or x.shape[1] != need or shrink not in (1, 2, 4, 8):
        raise ValueError(f"payload of shape {np.shape(payload)} for {w}x{h} layout {layout} at 1/{shrink}: "
                         f"{need} bytes per image, shrink 1, 2, 4 or 8")
    n, ow, oh = x.shape[0], -(-w // shrink), -(-h // shrink)
    what = "mipx_op_jpegd_to_rgb_scaled"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x)
    b = 1 if layout == YCC_GREY else 3
    dout = _dev("out", what, n * oh * ow * b, ow * b)
    wsb = lib.mipx_op_workspace_bytes(OP_JPEGD, n, ow, oh, 3, 0.0, 0.0)
    ws = _dev("ws", what, wsb)
    check(lib.mipx_op_jpegd_to_rgb_scaled(din.ptr, dout.ptr, n, w, h, layout, shrink, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, ws)
    return dout.download((n, oh, ow, b))


def jpegh_bytes(w: int, h: int, layout: int) -> int:
    """mipx_jpegh_bytes: bytes of one image's entropy-coded input slot, the 1504 bytes of header and
    tables and jpegc_bytes of room for the scan (0 for bad arguments)."""
    return int(lib.mipx_jpegh_bytes(w, h, layout))


def _jpegh_slots(slots, w: int, h: int, layout: int) -> np.ndarray:
    x = np.ascontiguousarray(slots, dtype=np.uint8)
    if x.ndim == 1:
        x = x[None]
    need = jpegh_bytes(w, h, layout)
    if x.ndim != 2 or need == 0 or x.shape[1] != need:
        raise ValueError(f"slots of shape {np.shape(slots)} for {w}x{h} layout {layout}: {need} bytes per image")
    return x


def jpegh_to_jpegd(slots: np.ndarray, w: int, h: int, layout: int):
    """mipx_op_jpegh_to_jpegd on entropy-coded input slots (codec.jpeg_huff_slot), (bytes,) or
    (n, bytes) uint8; returns (payloads, status): (n, jpegd_bytes) uint8 as codec.decode_jpeg_coefs
    gives them, and (n,) uint32 of JPEGH_OK / JPEGH_UNSYNCED / JPEGH_BAD."""
    sync_tuning()
    x = _jpegh_slots(slots, w, h, layout)
    n, need = x.shape[0], jpegd_bytes(w, h, layout)
    what = "mipx_op_jpegh_to_jpegd"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x)
    dout = _dev("out", what, n * need, 128 * ((w + 7) // 8))
    dst = _dev("status", what, 4 * n)
    wsb = lib.mipx_op_workspace_bytes(OP_JPEGH, n, w, h, 3, 0.0, 0.0)
    ws = _dev("ws", what, wsb)
    check(lib.mipx_op_jpegh_to_jpegd(din.ptr, dout.ptr, dst.ptr, n, w, h, layout, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, dst, ws)
    return dout.download((n, need)), dst.download((n,), np.uint32)


def jpegh_to_rgb_scaled(slots: np.ndarray, w: int, h: int, layout: int, shrink: int, _full: bool = False):
    """mipx_op_jpegh_to_rgb_scaled on the entropy-coded input slots of w x h files; returns
    (pixels, status): (n, ceil(h / shrink), ceil(w / shrink), 3) uint8, unspecified where the
    status is not JPEGH_OK, and (n,) uint32."""
    sync_tuning()
    x = _jpegh_slots(slots, w, h, layout)
    if shrink not in (1, 2, 4, 8):
        raise ValueError(f"shrink {shrink}: 1, 2, 4 or 8")
    n, ow, oh = x.shape[0], -(-w // shrink), -(-h // shrink)
    what = "mipx_op_jpegh_to_rgb" if _full else "mipx_op_jpegh_to_rgb_scaled"
    din = _dev("in", what, x.nbytes, 128 * ((w + 7) // 8), x)
    b = 1 if layout == YCC_GREY else 3   # a grey file decodes to its one plane
    dout = _dev("out", what, n * oh * ow * b, ow * b)
    dst = _dev("status", what, 4 * n)
    wsb = lib.mipx_op_workspace_bytes(OP_JPEGH, n, w, h, 3, 0.0, 0.0)
    ws = _dev("ws", what, wsb)
    if _full:
        check(lib.mipx_op_jpegh_to_rgb(din.ptr, dout.ptr, dst.ptr, n, w, h, layout, ws.ptr, wsb, None), what)
    else:
        check(lib.mipx_op_jpegh_to_rgb_scaled(din.ptr, dout.ptr, dst.ptr, n, w, h, layout, shrink, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, dst, ws)
    return dout.download((n, oh, ow, b)), dst.download((n,), np.uint32)


def jpegh_to_rgb(slots: np.ndarray, w: int, h: int, layout: int):
    """mipx_op_jpegh_to_rgb: as jpegh_to_rgb_scaled, at full size."""
    return jpegh_to_rgb_scaled(slots, w, h, layout, 1, _full=True)


def jpeg_roundtrip(imgs: np.ndarray, layout: int, quality: int, shrink: int = 1) -> np.ndarray:
    """mipx_op_jpeg_roundtrip on (h, w, 3) or (n, h, w, 3) uint8: the pixels the JPEG of each image
    at `quality` decodes to at 1/shrink; returns (n, ceil(h / shrink), ceil(w / shrink), 3)."""
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    if b != 3 or layout not in (YCC_444, YCC_420) or shrink not in (1, 2, 4, 8):
        raise ValueError(f"images of shape {np.shape(imgs)}, layout {layout} at 1/{shrink}: RGB, YCC_444 / YCC_420, "
                         f"shrink 1, 2, 4 or 8")
    ow, oh = -(-w // shrink), -(-h // shrink)
    what = "mipx_op_jpeg_roundtrip"
    din = _dev("in", what, x.nbytes, w * 3, x)
    dout = _dev("out", what, n * oh * ow * 3, ow * 3)
    wsb = lib.mipx_op_workspace_bytes(OP_JPEGRT, n, w, h, 3, float(shrink), 0.0)
    ws = _dev("ws", what, wsb)
    check(lib.mipx_op_jpeg_roundtrip(din.ptr, dout.ptr, n, w, h, layout, quality, shrink, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, ws)
    return dout.download((n, oh, ow, 3))


def smartcrop_origins(imgs: np.ndarray, cw: int, ch: int) -> np.ndarray:
    sync_tuning()
    x = _batch(imgs)
    n, h, w, b = x.shape
    what = "mipx_op_smartcrop_origin"
    din = _dev("in", what, x.nbytes, w * b, x)
    wsb = lib.mipx_op_workspace_bytes(7, n, w, h, b, cw, ch)
    ws = _dev("ws", what, wsb)
    org = _dev("origins", what, 8 * n)
    check(lib.mipx_op_smartcrop_origin(din.ptr, org.ptr, n, w, h, b, cw, ch, ws.ptr, wsb, None), what)
    synchronize()
    _check_guards(what, din, ws, org)
    return org.download((n, 2), np.int32)


def execute(plan: MipxPlan, imgs: np.ndarray, wm: Optional[np.ndarray] = None,
            junk: Optional[int] = None) -> np.ndarray:
    """mipx_execute_dev on a batch of host images (uploads, runs the plan, downloads); for a
    plan that takes planar input (plan_set_ycc_input), on packed planes, (bytes,) or (n, bytes),
    and for one that takes coefficient input (plan_set_jpegd_input[_scaled]), on payloads of the same shapes;
    a plan that gives coefficients (plan_set_jpegc_output) returns (n, jpegc_bytes / 2) int16, one
    that gives scans (plan_set_jpeg_scan_output) the slots, (n, jpeg_scan_bytes) uint8.
    junk: fill the workspace (the ping-pong intermediates) and the output with this byte
    first, so a step that reads outside what the steps before it wrote shows up."""
    sync_tuning()
    planar = _packed_input(plan)
    x = _planes(plan, imgs) if planar else _batch(imgs)
    n = x.shape[0]
    what = "mipx_execute_dev"
    din = _dev("in", what, x.nbytes, plan.in_w if planar else x.shape[2] * x.shape[3], x)
    coefs = _jpegc_layout(plan)
    scan = _jpege_layout(plan)
    out1 = jpegc_bytes(plan.out_w, plan.out_h, coefs) if coefs is not None else plan.out_w * plan.out_h * plan.out_bands
    if scan is not None:
        out1 = _jpege_slot_bytes(plan)
    dout = _dev("out", what, n * out1, plan.out_w * plan.out_bands)
    wsb = lib.mipx_workspace_bytes(C.byref(plan), n)
    ws = _dev("ws", what, wsb) if wsb else None
    if junk is not None:
        check(lib.mipx_memset_dev(dout.ptr, junk, dout.nbytes), "mipx_memset_dev")
        if ws:
            check(lib.mipx_memset_dev(ws.ptr, junk, ws.nbytes), "mipx_memset_dev")
    dwm = None
    if wm is not None:
        wm = np.ascontiguousarray(wm, dtype=np.uint8)
        dwm = _dev("wm", what, wm.nbytes, _wm_row_bytes(wm), wm)
    check(lib.mipx_execute_dev(C.byref(plan), n, din.ptr, dout.ptr, dwm.ptr if dwm else None,
                               ws.ptr if ws else None, wsb, None), what)
    synchronize()
    _check_guards(what, din, dout, dwm, ws)
    global _last_status
    _last_status = ws.download((n,), np.uint32) if _jpegh_layout(plan) is not None else None
    if coefs is not None:
        return dout.download((n, out1 // 2), np.int16)
    if scan is not None:
        return dout.download((n, out1))
    return dout.download((n, plan.out_h, plan.out_w, plan.out_bands))


_last_status = None


def execute_status():
    """The statuses (n uint32 of JPEGH_*) the last execute() of a plan with entropy-coded input
    (plan_set_jpegh_input[_scaled]) left at the head of its workspace; None after any other plan."""
    return _last_status


def _wm_row_bytes(wm: np.ndarray) -> int:
    return int(wm.shape[1] * (wm.shape[2] if wm.ndim == 3 else 1)) if wm.ndim >= 2 else int(wm.size)


def _vips_round(v: float) -> int:
    import math
    return int(math.ceil(v - 0.5)) if v < 0 else int(math.floor(v + 0.5))


def _osz_reduce(n: int, s: float) -> int:
    return _vips_round(n / s)


def _osz_shrink(n: int, s: int) -> int:
    return max(1, _vips_round(n / s))
