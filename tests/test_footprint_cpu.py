"""CPU side of the footprint checks: the damage report of a guard band, the rule that
every GPU module running kernels imports the guard fixture, and the share of
tests/test_footprint_gpu.py's generated cases that its rejection rule leaves out."""
import ast
import glob
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_CALLS = ("run_op", "execute", "smartcrop_origins")


def _damage(fill, before, after, nbytes):
    from imaginary_amd.engine import guard_damage
    return guard_damage(fill, np.asarray(before, np.uint8), np.asarray(after, np.uint8), nbytes)


def test_guard_damage_clean():
    assert _damage(0xA5, [0xA5] * 4096, [0xA5] * 4096, 207) is None
    assert _damage(0x5A, [0x5A] * 4099, [0x5A] * 4096, 1) is None


def test_guard_damage_one_byte_before():
    before = np.full(4096 + 3, 0xA5, np.uint8)
    before[-1] = 0
    assert _damage(0xA5, before, np.full(4096, 0xA5, np.uint8), 207) == (-1, -1, 1)
    before[:] = 0xA5
    before[0] = 0xA4   # the far end of the band
    assert _damage(0xA5, before, np.full(4096, 0xA5, np.uint8), 207) == (-4099, -4099, 1)


def test_guard_damage_run_after():
    after = np.full(4096, 0x5A, np.uint8)
    after[0:3] = (1, 2, 3)
    assert _damage(0x5A, np.full(4096, 0x5A, np.uint8), after, 207) == (207, 209, 3)
    after[2] = 0x5A    # a byte of the run that happens to equal the fill is not counted
    assert _damage(0x5A, np.full(4096, 0x5A, np.uint8), after, 207) == (207, 208, 2)


def test_guard_damage_both_bands():
    before = np.full(8192, 0xA5, np.uint8)
    after = np.full(8192, 0xA5, np.uint8)
    before[-16:] = 0
    after[60:64] = 0xFF
    assert _damage(0xA5, before, after, 1000) == (-16, 1063, 20)


def test_guard_width_rule():
    """G = 4096 * ceil((2 * row_bytes + 256) / 4096) for image buffers, 4096 otherwise
    (the allocation itself needs a device; the rule does not)."""
    from imaginary_amd.engine import GuardedBuffer
    for row_bytes, g in ((0, 4096), (1, 4096), (1920, 4096), (1921, 8192), (3840 * 3, 24576)):
        assert GuardedBuffer.guard_bytes(row_bytes) == g


def _engine_calls_and_import(path):
    tree = ast.parse(open(path).read(), path)
    calls, imported = [], False
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module == "footprint":
            imported |= any(a.name == "guarded" for a in node.names)
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Name) and f.id in ENGINE_CALLS:
            calls.append((f.id, node.lineno))
        elif isinstance(f, ast.Attribute) and f.attr in ENGINE_CALLS:
            # oracle.execute(...) / o.execute(...) is the CPU checker, not the engine
            if f.attr == "execute" and isinstance(f.value, ast.Name) and f.value.id in ("oracle", "o"):
                continue
            calls.append((f.attr, node.lineno))
    return calls, imported


def test_gpu_modules_that_run_kernels_import_the_guard():
    """A tests/test_*_gpu.py that calls run_op, execute or smartcrop_origins must import
    the autouse fixture `guarded` from footprint: no module opts out silently."""
    modules = sorted(glob.glob(os.path.join(HERE, "test_*_gpu.py")))
    assert len(modules) >= 11
    guarded_modules = []
    for path in modules:
        calls, imported = _engine_calls_and_import(path)
        if calls:
            assert imported, (f"{os.path.basename(path)} calls {calls[0][0]} (line {calls[0][1]}) without "
                              "`from footprint import guarded  # noqa: F401`")
            guarded_modules.append(os.path.basename(path)[5:-7])
    for name in ("parity", "rcol", "bcol", "rstrip", "affine", "chain", "demand", "configs", "fuzz", "sampling",
                 "footprint"):
        assert name in guarded_modules, name


def test_scan_sees_a_module_that_opts_out(tmp_path):
    p = tmp_path / "test_new_gpu.py"
    p.write_text("def test_x(gpu):\n    gpu.run_op('bw', None)\n    oracle.execute(1, 2)\n")
    calls, imported = _engine_calls_and_import(str(p))
    assert calls == [("run_op", 2)] and not imported
    p.write_text("from footprint import guarded  # noqa: F401\n\ndef test_x(ia):\n    ia.execute(1, 2)\n")
    calls, imported = _engine_calls_and_import(str(p))
    assert calls == [("execute", 4)] and imported


def test_footprint_cases_skip_share():
    """At most 10 % of the generated (op, parameters, shape, bands, n) cases fall to the
    explicit rejection rule, and every case that runs has a geometry the oracle accepts."""
    import test_footprint_gpu as fg
    assert fg.GENERATED > 2000
    assert fg.SKIPPED * 10 <= fg.GENERATED, (fg.SKIPPED, fg.GENERATED)
    ran = sum(len(p.values[2]) for p in fg.REDUCE_GROUPS + fg.OP_GROUPS)
    assert ran == fg.GENERATED - fg.SKIPPED
    # the rule agrees with the oracle's own size rules on the reduce family
    from oracle import oracle as o
    o.build()
    for p in fg.REDUCE_GROUPS + fg.OP_GROUPS:
        op, params, cases = p.values
        if op not in ("reduce", "reducev", "reduceh", "extract"):
            continue
        for h, w, b, n in cases:
            kw = fg.resolve(op, params, h, w, b)
            fg.oracle_op(o, op, kw, np.zeros((h, w, b), np.uint8))   # raises OracleError on a refused geometry
    for op, params, h, w in (("reduce", dict(hshrink=2.5, vshrink=1.0), 1, 1), ("reducev", dict(vshrink=3.3), 1, 7)):
        assert fg.rejected(op, params, h, w, 3)
        try:
            fg.oracle_op(o, op, fg.resolve(op, params, h, w, 3), np.zeros((h, w, 3), np.uint8))
        except o.OracleError:
            continue
        raise AssertionError(f"the oracle accepts {op} {params} on {h}x{w}, the rule rejects it")


# ---------------------------------------------------------------- the plumbing, on a host stand-in for the device
class _HostLib:
    """Stands in for libmipx's memory helpers and two entry points with host memory, and
    records every call: run_op's buffer handling can then be checked without a device.
    `stray` makes the rot entry point write one byte at that offset from its output."""

    def __init__(self, stray=None):
        import ctypes as C
        self.C, self.calls, self.live, self.stray = C, [], {}, stray

    def mipx_dev_malloc(self, ref, n):
        buf = (self.C.c_ubyte * n)()
        self.live[self.C.addressof(buf)] = buf
        ref._obj.value = self.C.addressof(buf)
        self.calls.append(("malloc", n))
        return 0

    def mipx_dev_free(self, p):
        self.calls.append(("free",))
        del self.live[p]
        return 0

    def mipx_memset_dev(self, p, v, n):
        self.calls.append(("memset", v, n))
        self.C.memset(p, v, n)
        return 0

    def mipx_memcpy_h2d(self, d, s, n):
        self.calls.append(("h2d", n))
        self.C.memmove(d, s, n)
        return 0

    def mipx_memcpy_d2h(self, d, s, n):
        self.calls.append(("d2h", n))
        self.C.memmove(d, s, n)
        return 0

    def mipx_device_sync(self):
        self.calls.append(("sync",))
        return 0

    def mipx_op_rot(self, din, dout, n, w, h, b, angle, stream):
        assert angle == 0
        self.calls.append(("rot", n * w * h * b))
        self.C.memmove(dout, din, n * w * h * b)
        if self.stray is not None:
            self.C.memset(dout + self.stray, 0x11, 1)
        return 0


def _with_host_lib(monkeypatch, stray=None):
    from imaginary_amd import engine
    fake = _HostLib(stray)
    monkeypatch.setattr(engine, "lib", fake)
    monkeypatch.setattr(engine, "sync_tuning", lambda: None)
    return engine, fake


def test_guard_off_makes_the_plain_calls(monkeypatch):
    """Off (the default): exact-size allocations, no memset, no guard downloads."""
    engine, fake = _with_host_lib(monkeypatch)
    assert engine.guard_setting() is None
    x = np.arange(2 * 3 * 5 * 3, dtype=np.uint8).reshape(2, 3, 5, 3)
    before = engine.guarded_calls()
    assert np.array_equal(engine.run_op("rot", x, angle=0), x)
    assert engine.guarded_calls() == before
    assert [c for c in fake.calls if c[0] != "free"] == [("malloc", 90), ("h2d", 90), ("malloc", 90), ("rot", 90),
                                                         ("sync",), ("d2h", 90)]


def test_guard_on_guards_poisons_and_checks(monkeypatch):
    engine, fake = _with_host_lib(monkeypatch)
    x = np.arange(2 * 3 * 5 * 3, dtype=np.uint8).reshape(2, 3, 5, 3)
    prev = engine.set_guard(0x5A, 3, 1)
    try:
        assert prev == (None, 0, 0) and engine.guard_setting() == (0x5A, 3, 1)
        before = engine.guarded_calls()
        assert np.array_equal(engine.run_op("rot", x, angle=0), x)
        assert engine.guarded_calls() == before + 1
    finally:
        assert engine.set_guard(*prev) == (0x5A, 3, 1)
    assert engine.guard_setting() is None
    assert [c for c in fake.calls if c[0] != "free"] == [
        ("malloc", 4096 + 3 + 90 + 4096), ("memset", 0x5A, 4096 + 3 + 90 + 4096), ("h2d", 90),
        ("malloc", 4096 + 1 + 90 + 4096), ("memset", 0x5A, 4096 + 1 + 90 + 4096), ("rot", 90), ("sync",),
        ("d2h", 4096 + 3), ("d2h", 4096), ("d2h", 4096 + 1), ("d2h", 4096), ("d2h", 90)]


def test_run_op_names_buffer_op_and_offset_of_a_stray_write(monkeypatch):
    x = np.arange(90, dtype=np.uint8).reshape(1, 6, 5, 3)
    for stray in (90, 92, -1, -4096):
        engine, fake = _with_host_lib(monkeypatch, stray)
        prev = engine.set_guard(0xA5)
        try:
            with pytest.raises(AssertionError) as e:
                engine.run_op("rot", x, angle=0)
        finally:
            engine.set_guard(*prev)
        msg = str(e.value)
        assert "mipx_op_rot" in msg and "'out'" in msg and "1 byte(s)" in msg, msg
        assert f"first at payload offset {stray}, last at {stray} " in msg, msg
