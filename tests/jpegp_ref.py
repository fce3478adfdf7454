"""The reference of packed scan slots (mipx_op_*_scan_packed, include/mipx.h): the slots of
jpege_ref.slot_ref (head 16) or jpegeo_ref.slot_ref (head 1104) back to back, each rounded up to 16
bytes, behind a directory of n + 1 byte offsets:

    off[0] = 0,  off[i + 1] = off[i] + align16(head + (status_i == OK ? length_i : 0))

A slot that is OVERFLOW or UNCODABLE is its header alone; an OVERFLOW header's length is a need above
the capacity and means no bytes.  Where the interface leaves a byte open (the `bits` word of an
UNCODABLE header, the tables of a slot that is not OK, the pads) pack_ref writes 0 and check_packed
does not compare."""
import numpy as np

import jpege_ref
import jpegeo_ref
from jpege_ref import OK

HEADS = (16, 1104)
FILL = 0xA5


def align16(v):
    return (v + 15) // 16 * 16


def slot_span(slot, head):
    """Bytes of one packed slot that are written: the header, and the scan when there is one."""
    return head + (slot.length if slot.status == OK else 0)


def slot_bytes_ref(slot, head):
    """One slot's written bytes as uint8."""
    out = np.zeros(slot_span(slot, head), np.uint8)
    out[:16] = np.array([slot.length, slot.status, slot.bits or 0, 1 if head == 1104 else 0], "<u4").view(np.uint8)
    if slot.status == OK:
        if head == 1104:
            for k, tc in enumerate(jpegeo_ref.SLOT_TABLES):
                out[16 + 272 * k:16 + 272 * (k + 1)] = jpegeo_ref.table_bytes(slot.tables[tc])
        out[head:] = np.frombuffer(slot.scan, np.uint8)
    return out


def dir_ref(slots, head):
    """The directory alone: n + 1 uint64 byte offsets."""
    assert head in HEADS
    off = [0]
    for s in slots:
        off.append(off[-1] + align16(slot_span(s, head)))
    return np.array(off, "<u8")


def pack_ref(slots, head):
    """(dir, bytes): the n + 1 uint64 offsets and the off[n] bytes they describe."""
    off = dir_ref(slots, head)
    data = np.zeros(int(off[-1]), np.uint8)
    for i, s in enumerate(slots):
        b = slot_bytes_ref(s, head)
        data[int(off[i]):int(off[i]) + b.size] = b
    return off, data


def check_packed(got_dir, got, slots, head, what, fill=FILL):
    """A downloaded directory and output buffer (that started out all `fill`) against the reference:
    the directory, each slot by its own check_slot over [off[i], off[i] + head + length_i), and every
    other byte of the buffer, the pads and all from off[n] on, still `fill`."""
    check_slot = jpegeo_ref.check_slot if head == 1104 else jpege_ref.check_slot
    want_dir = dir_ref(slots, head)
    got_dir = np.asarray(got_dir, dtype="<u8")
    assert got_dir.tolist() == want_dir.tolist(), f"{what}: directory {got_dir.tolist()[:8]}, want {want_dir.tolist()[:8]}"
    got = np.ascontiguousarray(got, dtype=np.uint8).ravel()
    assert int(want_dir[-1]) <= got.size, (what, int(want_dir[-1]), got.size)
    untouched = np.ones(got.size, bool)
    for i, s in enumerate(slots):
        a, span = int(want_dir[i]), slot_span(s, head)
        check_slot(got[a:a + span], s, f"{what}, slot {i}")
        if s.status == OK:   # check_slot stops at the header of the others: compare every written byte of these
            assert np.array_equal(got[a:a + span], slot_bytes_ref(s, head)), f"{what}, slot {i}: bytes differ"
        untouched[a:a + span] = False
    stray = np.flatnonzero(untouched & (got != fill))
    assert stray.size == 0, (f"{what}: {stray.size} byte(s) written outside the slots' headers and scans, the first at "
                             f"{int(stray[0])} (off[n] = {int(want_dir[-1])}, buffer {got.size})")
