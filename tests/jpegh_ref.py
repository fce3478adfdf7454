"""The reference of the entropy-coded JPEG input (MIPX_OP_JPEGH, PARITY_ASSUMPTIONS.md row 22): the
input slot restated (build_slot / parse_slot, and file_tables, a marker walk of its own), the sizes
include/mipx.h states in words, and the model of the device's decoder: which status a slot gets, and
the payload of MIPX_OP_JPEGD it decodes to.

The device starts one decoder per SUB bytes of unstuffed scan; the decoders of one sequence (SEQ of
them) run until their states agree, so a sequence behaves as one sequential decoder D_j from its
entry state.  Sequence 0 starts with the truth, sequence j > 0 with the guess (its first bit, block
0 of the MCU, zigzag index 0):  X_j^0 = D_j(guess),  X_j^r = D_j(X_(j-1)^(r-1)),  and the scan is
synchronised iff X^ROUNDS == X^(ROUNDS-1) for every sequence.  The rules of D are total:
  an unknown code skips one bit; a run and size that pass coefficient 63 end the block (the value
  bits stay unread); a DC symbol counts as symbol & 15 bits; sixteen zeros that pass 63 end the block.
On the verified path the first three, inside the scan's blocks, make the slot BAD, and so does a
block that ends behind the stream's last bit: what codec.decode_jpeg_coefs declines."""
import functools

import numpy as np

from jpegc_ref import YCC_420, YCC_444, jpegc_bytes
from jpege_ref import scan_blocks  # noqa: F401  (blocks of the scan, dummy blocks included)

HEADER_BYTES = 1504
JPEGD_HEADER_BYTES = 384
OK, UNSYNCED, BAD = 0, 1, 2
SUB, SEQ, ROUNDS = 128, 256, 2   # kJpeghSub bytes per lane, kJpeghSeq lanes per workgroup, kJpeghRounds launches more
SEQ_BYTES = SUB * SEQ
TABLE_KEYS = (0x00, 0x01, 0x10, 0x11)   # the slot's four tables by DHT Tc/Th byte: DC 0, DC 1, AC 0, AC 1
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)


def jpegh_bytes(w, h, layout):
    """mipx_jpegh_bytes: the header and the capacity, which is the coefficients' size."""
    n = jpegc_bytes(w, h, layout)
    return HEADER_BYTES + n if n else 0


def jpegd_bytes(w, h, layout):
    n = jpegc_bytes(w, h, layout)
    return JPEGD_HEADER_BYTES + n if n else 0


def workspace_bytes(n, w, h):
    """mipx_op_workspace_bytes(MIPX_OP_JPEGH, n, w, h, 3, 0, 0): sized without the layout.  Per image
    cap = the 4:4:4 coefficients, blocks = the scan's of whichever layout has more.  Parts, each
    rounded up to 256 bytes: the statuses (4 n), the per-image records (32 n), the unstuffed scans
    (n times cap + 8 rounded up), the stuffed-zero counts per 1024 bytes of scan and their scan
    (4 + 4), per subsequence of whole sequences an entry state and a block count (8 + 4), per
    sequence two exit states, a block count and its scan (16 + 4 + 4), a DC difference per block
    (4), per tile of 256 blocks three sums and their scans (12 + 24), the payloads of
    MIPX_OP_JPEGD (n (384 + cap)) and its planes (3 n w h)."""
    def up(v):
        return (v + 255) // 256 * 256
    cap = jpegc_bytes(w, h, YCC_444)
    blocks = max(scan_blocks(w, h, YCC_444), scan_blocks(w, h, YCC_420))
    tiles, chunks, seqs = -(-blocks // SEQ), -(-cap // (4 * SEQ)), -(-cap // SEQ_BYTES)
    return (up(4 * n) + up(32 * n) + n * up(cap + 8) + 2 * up(4 * n * chunks) + up(8 * n * seqs * SEQ)
            + up(4 * n * seqs * SEQ) + up(16 * n * seqs) + 2 * up(4 * n * seqs) + up(4 * n * blocks)
            + up(12 * n * tiles) + up(24 * n * tiles) + up(n * (384 + cap)) + up(3 * n * w * h))


# ---- the slot ---------------------------------------------------------------------------------
def build_slot(w, h, layout, scan, qtables, selectors, tables, length=None):
    """One input slot, uint8 of jpegh_bytes: scan the stuffed entropy-coded bytes; qtables three
    tables of 64 values in natural order (Y, Cb, Cr); selectors the DC table index of Y, Cb, Cr,
    then the AC table index of Y, Cb, Cr; tables {Tc/Th byte: (16 counts, symbols)} for some of
    TABLE_KEYS.  length: what the header says, when that is not len(scan)."""
    slot = np.zeros(jpegh_bytes(w, h, layout), np.uint8)
    assert len(scan) <= slot.size - HEADER_BYTES
    slot[0:4] = np.array([len(scan) if length is None else length], "<u4").view(np.uint8)
    slot[16:400] = np.asarray(qtables, "<u2").reshape(192).view(np.uint8)
    slot[400:406] = list(selectors)
    for i, key in enumerate(TABLE_KEYS):
        if key in tables:
            counts, symbols = tables[key]
            assert len(counts) == 16 and len(symbols) <= 256
            slot[416 + 272 * i:432 + 272 * i] = list(counts)
            slot[432 + 272 * i:432 + 272 * i + len(symbols)] = list(symbols)
    slot[HEADER_BYTES:HEADER_BYTES + len(scan)] = np.frombuffer(bytes(scan), np.uint8)
    return slot


def parse_slot(slot):
    """(length, qtables (3, 64), selectors [6], tables [4] of (counts bytes, 256 symbols bytes))."""
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    length = int(slot[0:4].view("<u4")[0])
    q = slot[16:400].view("<u2").reshape(3, 64).astype(int)
    tables = [(bytes(slot[416 + 272 * i:432 + 272 * i]), bytes(slot[432 + 272 * i:688 + 272 * i])) for i in range(4)]
    return length, q, slot[400:406].tolist(), tables


def file_tables(buf):
    """A baseline JPEG's headers by a marker walk of its own: (w, h, sampling [(h, v)] per component,
    qtables per component in natural order, selectors, {Tc/Th: (counts, symbols)}, restart interval,
    the bytes between the SOS segment and the marker that ends the scan)."""
    p, qt, dht, frame, dri = 2, {}, {}, None, 0
    while True:
        assert buf[p] == 0xFF
        m, size = buf[p + 1], int.from_bytes(buf[p + 2:p + 4], "big")
        body = buf[p + 4:p + 2 + size]
        p += 2 + size
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = body[1 + k]
                qt[body[0]] = t
                body = body[65:]
        elif m == 0xC4:
            while body:
                cnt = sum(body[1:17])
                dht[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + cnt]))
                body = body[17 + cnt:]
        elif m in (0xC0, 0xC1):
            frame = body
        elif m == 0xDD:
            dri = int.from_bytes(body, "big")
        elif m == 0xDA:
            sos = body
            break
    h, w, nc = int.from_bytes(frame[1:3], "big"), int.from_bytes(frame[3:5], "big"), frame[5]
    comps = [(frame[6 + 3 * i], frame[7 + 3 * i] >> 4, frame[7 + 3 * i] & 15, frame[8 + 3 * i]) for i in range(nc)]
    sel = [sos[2 + 2 * i] >> 4 for i in range(nc)] + [sos[2 + 2 * i] & 15 for i in range(nc)]
    end = p
    while not (buf[end] == 0xFF and buf[end + 1] != 0x00):
        end += 1
    return w, h, [(c[1], c[2]) for c in comps], [qt[c[3]] for c in comps], sel, dht, dri, bytes(buf[p:end])


# ---- the model ------------------------------------------------------------------------------------
def unstuff(scan):
    """(the scan without the 00 of every FF 00, whether an FF stands without one)."""
    scan = bytes(scan)
    out, i, n, marker = bytearray(), 0, len(scan), False
    while i < n:
        b = scan[i]
        out.append(b)
        i += 1
        if b == 0xFF:
            if i < n and scan[i] == 0x00:
                i += 1
            else:
                marker = True
    return bytes(out), marker


def lookup16(counts, symbols):
    """By the next 16 bits: length << 8 | symbol, 0 where no code matches; None for counts that are
    no Huffman table (more than 256 codes, or a code past its length's range)."""
    if sum(counts) > 256:
        return None
    lut, code, k = [0] * 65536, 0, 0
    for length in range(1, 17):
        c = counts[length - 1]
        if c:
            if code + c > 1 << length:
                return None
            for _ in range(c):
                lo = code << (16 - length)
                lut[lo:lo + (1 << (16 - length))] = [length << 8 | symbols[k]] * (1 << (16 - length))
                code += 1
                k += 1
        code <<= 1
    return lut


class Stream:
    """An unstuffed scan with its tables: what a decoder of the model needs."""

    def __init__(self, data, luts, selectors, layout, blocks):
        self.data = data + bytes(8)    # bits behind the stream read 0
        self.total = 8 * len(data)
        self.per_mcu = 3 if layout == YCC_444 else 6
        comp = [0, 1, 2] if layout == YCC_444 else [0, 0, 0, 0, 1, 2]
        self.dc = [luts[selectors[c]] for c in comp]
        self.ac = [luts[2 + selectors[3 + c]] for c in comp]
        self.blocks = blocks
        self.nsub = -(-len(data) // SUB)
        self.nseq = -(-self.nsub // SEQ)

    def run(self, pos, b, k, limit, cur=None, dcdiff=None, put=None):
        """Steps from state (pos, b, k) while pos < limit.  Returns (pos, b, k, blocks completed, bad).
        With cur (the block the state is in): stops when the scan's blocks are done, records DC
        differences and calls put(block, k, value) for AC values, and reports the rule breaks."""
        data, total, per_mcu, write = self.data, self.total, self.per_mcu, cur is not None
        done, bad = 0, False
        while pos < limit and (not write or cur < self.blocks):
            v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "big") >> (32 - (pos & 7))) & 0xFFFFFFFF
            e = (self.dc[b] if k == 0 else self.ac[b])[v >> 16]
            if e == 0:
                pos += 1
                bad = True
                continue
            ln, sym = e >> 8, e & 255
            size, end, at = sym & 15, False, -1
            if k == 0:
                bad = bad or sym > 15
                at, k = 0, 1
            elif size == 0:
                if sym >> 4 == 15:
                    k += 16
                    end = k > 63
                else:
                    end = True
            else:
                k += sym >> 4
                if k > 63:
                    bad = end = True
                else:
                    at = k
                    k += 1
                    end = k > 63
            pos += ln
            if at >= 0:
                if write:
                    val = 0
                    if size:
                        val = (v >> (32 - ln - size)) & ((1 << size) - 1)
                        if val < 1 << (size - 1):
                            val -= (1 << size) - 1
                    if at == 0:
                        dcdiff[cur] = val
                    elif val:
                        put(cur, at, val)
                pos += size
            if pos > total:
                bad = True
            if end:
                k = 0
                b = b + 1 if b + 1 < per_mcu else 0
                done += 1
                if write:
                    cur += 1
        return pos, b, k, done, bad


def synchronised(s):
    """Whether the device's launches agree on every sequence's exit state."""
    if s.nseq <= 1:
        return True
    seq_bits = 8 * SEQ_BYTES

    @functools.lru_cache(maxsize=None)
    def d(j, entry):
        return s.run(*entry, min((j + 1) * seq_bits, s.total))[:3]

    x = [d(0, (0, 0, 0))] + [d(j, (j * seq_bits, 0, 0)) for j in range(1, s.nseq)]
    for _ in range(ROUNDS):
        prev, x = x, [d(0, (0, 0, 0))] + [d(j, x[j - 1]) for j in range(1, s.nseq)]
    return x == prev


def block_place(w, h, layout):
    """Per block of the scan (component, index of the block among the component's real blocks in
    raster order, or -1 for a dummy block)."""
    ywb, yhb = (w + 7) // 8, (h + 7) // 8
    out = []
    if layout == YCC_444:
        for m in range(ywb * yhb):
            out += [(0, m), (1, m), (2, m)]
        return out
    mw, mh = ((w + 1) // 2 + 7) // 8, ((h + 1) // 2 + 7) // 8
    for my in range(mh):
        for mx in range(mw):
            for j in range(4):
                by, bx = 2 * my + (j >> 1), 2 * mx + (j & 1)
                out.append((0, by * ywb + bx if by < yhb and bx < ywb else -1))
            out += [(1, my * mw + mx), (2, my * mw + mx)]
    return out


def decode_slot(slot, w, h, layout):
    """(status, payload): the status the device gives the slot, and for OK the payload of
    MIPX_OP_JPEGD (uint8, jpegd_bytes) it must write; None otherwise."""
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    cap = jpegc_bytes(w, h, layout)
    assert slot.size == HEADER_BYTES + cap
    length, _, selectors, tables = parse_slot(slot)
    if length > cap or any(v > 1 for v in selectors):
        return BAD, None
    data, marker = unstuff(slot[HEADER_BYTES:HEADER_BYTES + length].tobytes())
    luts = [lookup16(c, sy) for c, sy in tables]
    if marker or any(t is None for t in luts):
        return BAD, None
    blocks = scan_blocks(w, h, layout)
    s = Stream(data, luts, selectors, layout, blocks)
    if not synchronised(s):
        return UNSYNCED, None
    place = block_place(w, h, layout)
    assert len(place) == blocks
    sizes = [max(i for c, i in place if c == comp) + 1 for comp in range(3)]
    assert 128 * sum(sizes) == cap
    coefs = [np.zeros((n, 64), np.int64) for n in sizes]
    dcdiff = [0] * blocks

    def put(cur, k, val):
        comp, i = place[cur]
        if i >= 0:
            coefs[comp][i, ZIGZAG[k]] = val

    _, _, _, done, bad = s.run(0, 0, 0, s.total, 0, dcdiff, put)
    if bad or done < blocks:
        return BAD, None
    pred = [0, 0, 0]
    for cur, (comp, i) in enumerate(place):
        pred[comp] += dcdiff[cur]
        if i >= 0:
            if not -32768 <= pred[comp] <= 32767:
                return BAD, None
            coefs[comp][i, 0] = pred[comp]
    body = np.concatenate([c.astype("<i2").ravel() for c in coefs]).view(np.uint8)
    return OK, np.concatenate([slot[16:400], body])


# ---- inputs -----------------------------------------------------------------------------------------
def dense_coefs(w, h):
    """4:4:4, every block DC 0 and all 63 AC coefficients 1: a scan without a single end-of-block
    code, every block 191 bits with the Annex K tables.  A decoder that starts inside it at a wrong
    zigzag index never finds the right one, so such a scan is decoded one subsequence per pass."""
    c = np.ones((3 * ((w + 7) // 8) * ((h + 7) // 8), 64), np.int16)
    c[:, 0] = 0
    return c.reshape(-1)


def dense_size(sequences):
    """The smallest square size, a multiple of 8, whose dense scan spans more than `sequences` sequences."""
    side = 8
    while 3 * (side // 8) ** 2 * 191 <= 8 * SEQ_BYTES * sequences:
        side += 8
    return side
