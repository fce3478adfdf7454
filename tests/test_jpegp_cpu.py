"""Packed scan slots without a GPU: the new symbols and their refusals, mipx_jpeg_scan_unpack (the one
piece of host logic that writes a caller's buffer by a length the device reported) on hand-made
buffers, and the packing rule's own properties (tests/jpegp_ref.py)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import jpege_ref
import jpegeo_ref
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpege_ref import OK, OVERFLOW, UNCODABLE
from jpegp_ref import FILL, HEADS, align16, dir_ref, pack_ref, slot_span
from test_abi import HEADER

EINVAL, ENOTINIT, EDATA = -1, -7, -10
W, H = 16, 16


def _slot_ref(head):
    return jpegeo_ref.slot_ref if head == 1104 else jpege_ref.slot_ref


def _slot_size(head, w, h, layout):
    return head + jpegc_bytes(w, h, layout)


@functools.lru_cache(maxsize=None)
def three(layout):
    """Coefficients of three 16 x 16 images whose slots are OK, OVERFLOW and UNCODABLE (the recipes of
    tests/test_jpege_gpu.py)."""
    px = np.random.default_rng(7).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    c = jpegc_ref(px, layout, 90).copy()
    c[1] = np.where(np.arange(c.shape[1]) % 2 == 0, 1023, -1023)
    c[1, ::64] = 0
    c[2, 0] = 2048
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def three_slots(layout, head):
    s = [_slot_ref(head)(x, W, H, layout) for x in three(layout)]
    if head == 1104:
        # no coefficients are known that overflow with optimised tables (tests/test_jpegeo_gpu.py): the
        # header is made by hand, as the kernels would report it
        need = jpegc_bytes(W, H, layout) + 37
        s[1] = jpegeo_ref.Slot(need, OVERFLOW, 8 * need - 3, b"", None)
    assert [x.status for x in s] == [OK, OVERFLOW, UNCODABLE]
    return tuple(s)


def _unpack(ia, d, packed, i, head, slot_bytes, packed_bytes=None):
    d = np.ascontiguousarray(d, dtype="<u8")
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    slot = np.full(slot_bytes, FILL, np.uint8)
    e = ia.lib.mipx_jpeg_scan_unpack(d.ctypes.data, d.size - 1, packed.ctypes.data,
                                     packed.size if packed_bytes is None else packed_bytes, i, head, slot.ctypes.data,
                                     slot.size)
    return e, slot


# ---------------------------------------------------------------- the symbols
def test_the_new_symbols_are_declared_and_the_abi_version_stays():
    import imaginary_amd as ia
    from imaginary_amd._abi import _SIG
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    for decl in (
            "int mipx_op_jpegc_to_scan_packed(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h, "
            "int32_t layout, void *d_work, void *stream, int32_t optimize, uint64_t *d_dir);",
            "int mipx_op_rgb_to_jpeg_scan_packed(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, "
            "int32_t layout, int32_t quality, void *d_work, void *stream, int32_t optimize, uint64_t *d_dir);",
            "size_t mipx_jpeg_scan_packed_dir_bytes(int32_t n);",
            "int mipx_jpeg_scan_unpack(const uint64_t *dir, int32_t n, const uint8_t *packed, size_t packed_bytes, "
            "int32_t i, size_t head, uint8_t *slot, size_t slot_bytes);",
            "int mipx_transfer_stats(int queue, uint64_t *h2d_bytes, uint64_t *d2h_bytes);"):
        assert decl in flat, decl
    for name, nargs in (("mipx_op_jpegc_to_scan_packed", 10), ("mipx_op_rgb_to_jpeg_scan_packed", 11),
                        ("mipx_jpeg_scan_packed_dir_bytes", 1), ("mipx_jpeg_scan_unpack", 8), ("mipx_transfer_stats", 3)):
        assert hasattr(ia.lib, name) and len(_SIG[name][1]) == nargs, name
    assert ia.lib.mipx_abi_version() == 6
    assert [ia.lib.mipx_jpeg_scan_packed_dir_bytes(n) for n in (1, 3, 300)] == [16, 32, 2408]
    for name in ("rgb_to_jpeg_scan_packed", "jpegc_to_scan_packed", "scan_unpack"):
        assert callable(getattr(ia, name))
    assert callable(ia.Engine.transfer_stats)


def test_transfer_stats_before_init():
    import imaginary_amd as ia
    ia.lib.mipx_shutdown()
    a, b = C.c_uint64(), C.c_uint64()
    assert ia.lib.mipx_transfer_stats(0, C.byref(a), C.byref(b)) == ENOTINIT
    assert ia.lib.mipx_transfer_stats(0, None, None) == ENOTINIT


def test_packed_ops_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    f, g = ia.lib.mipx_op_rgb_to_jpeg_scan_packed, ia.lib.mipx_op_jpegc_to_scan_packed
    P = 4096   # a "device pointer": 16-byte aligned, never used
    for opt in (0, 1):
        assert f(None, P, 1, 8, 8, YCC_420, 75, P, None, opt, P) == EINVAL
        assert f(P, None, 1, 8, 8, YCC_420, 75, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, YCC_420, 75, None, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, YCC_420, 75, P, None, opt, None) == EINVAL
        assert f(P, P, 0, 8, 8, YCC_420, 75, P, None, opt, P) == EINVAL
        assert f(P, P, -1, 8, 8, YCC_444, 75, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 0, 8, YCC_420, 75, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, 2, 75, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, -1, 75, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, YCC_420, 0, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, YCC_420, 101, P, None, opt, P) == EINVAL
        assert f(P, P, 1, 8, 8, YCC_420, 75, P + 4, None, opt, P) == EINVAL    # a misaligned workspace
        assert f(P, P, 1, 8, 8, YCC_420, 75, P, None, opt, P + 4) == EINVAL    # a misaligned directory
        assert g(None, P, 1, 8, 8, YCC_420, P, None, opt, P) == EINVAL
        assert g(P, None, 1, 8, 8, YCC_420, P, None, opt, P) == EINVAL
        assert g(P, P, 1, 8, 8, YCC_420, None, None, opt, P) == EINVAL
        assert g(P, P, 1, 8, 8, YCC_420, P, None, opt, None) == EINVAL
        assert g(P, P, 0, 8, 8, YCC_420, P, None, opt, P) == EINVAL
        assert g(P, P, 1, 8, 0, YCC_420, P, None, opt, P) == EINVAL
        assert g(P, P, 1, 8, 8, 2, P, None, opt, P) == EINVAL
        assert g(P, P, 1, 8, 8, YCC_444, P, None, opt, P + 2) == EINVAL
    assert f(P, P, 1, 8, 8, YCC_420, 75, P, None, 2, P) == EINVAL              # optimize is 0 or 1
    assert g(P, P, 1, 8, 8, YCC_420, P, None, -1, P) == EINVAL


# ---------------------------------------------------------------- mipx_jpeg_scan_unpack
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
def test_unpack_round_trips_the_reference(layout, head):
    import imaginary_amd as ia
    a, b, c = three_slots(layout, head)
    size = _slot_size(head, W, H, layout)
    for mix in ([a], [a, b, a], [b, c], [c, a, b, a, c], [a, a, a]):
        d, packed = pack_ref(mix, head)
        room = np.full(packed.size + 64, 0x3C, np.uint8)    # the buffer may be larger than off[n]
        room[:packed.size] = packed
        for i, s in enumerate(mix):
            e, slot = _unpack(ia, d, room, i, head, size)
            assert e == 0
            span = slot_span(s, head)
            assert np.array_equal(slot[:span], packed[int(d[i]):int(d[i]) + span]), (i, s.status)
            assert (slot[span:] == FILL).all(), "bytes behind the header and the scan were written"
            if s.status == OK:
                (jpegeo_ref.check_slot if head == 1104 else jpege_ref.check_slot)(slot, s, f"slot {i}")
                assert np.array_equal(ia.scan_unpack(d, room, i, head, size), slot)
            else:
                assert span == head
        # a destination of exactly the bytes needed is enough
        e, slot = _unpack(ia, d, room, 0, head, slot_span(mix[0], head))
        assert e == 0 and np.array_equal(slot, packed[:slot.size])


@pytest.mark.parametrize("head", HEADS)
def test_an_overflow_header_of_any_length_copies_the_header_only(head):
    import imaginary_amd as ia
    a, b, _ = three_slots(YCC_420, head)
    assert b.length > jpegc_bytes(W, H, YCC_420)
    d, packed = pack_ref([b, a], head)
    assert int(d[1]) == head
    packed[:4] = 0xFF   # length 0xffffffff
    e, slot = _unpack(ia, d, packed, 0, head, _slot_size(head, W, H, YCC_420))
    assert e == 0 and np.array_equal(slot[:head], packed[:head]) and (slot[head:] == FILL).all()
    e, slot = _unpack(ia, d, packed, 0, head, head)
    assert e == 0 and np.array_equal(slot, packed[:head])


@pytest.mark.parametrize("head", HEADS)
def test_each_inconsistency_is_edata_and_writes_nothing(head):
    import imaginary_amd as ia
    a, b, c = three_slots(YCC_444, head)
    size = _slot_size(head, W, H, YCC_444)
    d, packed = pack_ref([a, b, a], head)
    step = int(d[1])
    assert step == align16(head + a.length) and int(d[2]) == step + head

    def refused(dd, i=0, packed_bytes=None, slot_bytes=size, data=packed):
        e, slot = _unpack(ia, dd, data, i, head, slot_bytes, packed_bytes)
        assert e == EDATA and (slot == FILL).all(), (e, dd.tolist())

    for i in range(3):
        assert _unpack(ia, d, packed, i, head, size)[0] == 0
    bad = d.copy()
    bad[0] = 16
    refused(bad)                                        # off[0] is not 0
    bad = d.copy()
    bad[2] = bad[1] - 16
    refused(bad), refused(bad, i=2)                     # a decreasing step
    bad = d.copy()
    bad[1:] += 8
    refused(bad)                                        # a step that is no multiple of 16
    bad = d.copy()
    bad[2:] -= 16
    refused(bad), refused(bad, i=1)                     # a step below head (the OVERFLOW slot's: head - 16)
    refused(d, packed_bytes=int(d[3]) - 1)              # off[n] past packed_bytes
    long = packed.copy()
    long[:4] = np.array([step - head + 1], "<u4").view(np.uint8)
    refused(d, data=long)                               # an OK length past its step
    refused(d, slot_bytes=head + a.length - 1)          # an OK length past slot_bytes
    # ... and the arguments that are not data
    assert _unpack(ia, d, packed, 3, head, size)[0] == EINVAL
    assert _unpack(ia, d, packed, -1, head, size)[0] == EINVAL
    assert _unpack(ia, d, packed, 0, 32, size)[0] == EINVAL
    with pytest.raises(ia.MipxError):
        ia.scan_unpack(bad, packed, 0, head, size)


# ---------------------------------------------------------------- the packing rule
def test_packed_slots_never_need_more_than_the_slots():
    """head is a multiple of 16, the capacity one of 128, and an OK scan fits its capacity."""
    from test_jpege_gpu import SIZES
    for head in HEADS:
        assert head % 16 == 0
        for w, h in SIZES:
            for layout in (YCC_444, YCC_420):
                cap = jpegc_bytes(w, h, layout)
                assert cap % 128 == 0
                full = jpege_ref.Slot(cap, OK, 8 * cap, bytes(cap))     # only lengths and statuses enter the directory
                least = jpege_ref.Slot(1, OK, 1, b"\x7f")
                over = jpege_ref.Slot(2 * cap, OVERFLOW, 16 * cap, b"")
                assert align16(slot_span(full, head)) == head + cap
                for n in (1, 3):
                    for mix in ([full] * n, [least] * n, [over] * n, [full, over, least][:n]):
                        off = dir_ref(mix, head)
                        assert int(off[-1]) <= len(mix) * (head + cap), (w, h, layout, head)
                        assert (np.diff(off.astype(np.int64)) >= head).all()


@pytest.mark.parametrize("head", HEADS)
def test_a_batch_without_an_ok_slot_packs_to_its_headers(head):
    _, b, c = three_slots(YCC_420, head)
    for mix in ([b], [c], [b, c, c, b]):
        d, packed = pack_ref(mix, head)
        assert d.tolist() == [head * i for i in range(len(mix) + 1)] and packed.size == len(mix) * head
        for i, s in enumerate(mix):
            assert packed[head * i + 4:head * i + 8].view("<u4")[0] == s.status


# ---------------------------------------------------------------- the C driver
def test_c_driver_builds_against_the_header(tmp_path):
    """tests/c/mipx_e2e_scan.c, the request-path measurement with a scan answer, compiles cleanly
    against include/mipx.h and links mipx_transfer_stats; without a device it says so."""
    import os
    import subprocess
    from conftest import ROOT
    import imaginary_amd as ia
    exe = os.path.join(str(tmp_path), "mipx_e2e_scan")
    subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c11", "-D_DEFAULT_SOURCE",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "mipx_e2e_scan.c"),
                    "-L", os.path.join(ROOT, "imaginary_amd"), "-lmipx", "-lpthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "imaginary_amd"), "-o", exe], check=True)
    if ia.device_count() == 0:
        assert subprocess.run([exe, "scan", "1", "1"], capture_output=True).returncode == 77


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_unpack_in_a_program_of_its_own(tmp_path, sanitize):
    """tests/c/jpegp_unpack_host.cpp: the same function on heap buffers of exactly the stated sizes; with
    the sanitizers it is this program that runs under them, nothing loaded into Python."""
    import os
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "imaginary_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    exe = tmp_path / "jpegp_unpack_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"] +
                   (flags if sanitize else []) +
                   ["-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "jpegp_unpack_host.cpp"), os.path.join(csrc, "mipx_tables.cpp"),
                    os.path.join(csrc, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout[-2000:] + out.stderr[-2000:]
