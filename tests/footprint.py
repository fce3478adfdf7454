"""Footprint checking for the GPU tests: every device buffer a test hands to a kernel
sits between two guard bands and starts out poisoned.

A GPU test module that calls run_op, execute or smartcrop_origins imports the autouse
fixture below (`from footprint import guarded  # noqa: F401`; tests/test_footprint_cpu.py
fails for a module that does not).  Under it every such call allocates
engine.GuardedBuffer instead of exact-size buffers: input, output, watermark, workspace
and origins each lie inside their own 0xA5-filled allocation, output and workspace
payloads start as 0xA5, the workspace is exactly the advertised size, and every guard
is checked after the synchronise.  Each existing case so asserts, next to what it
asserted before, that the kernels wrote nothing outside the output and the advertised
workspace, and a kernel that leaves output bytes unwritten cannot pass on a zeroed or
stale buffer.

Known limits: a stray write further from a payload than the guard width (two rows + 256
bytes, rounded up to 4096) is not seen; and the ping-pong buffers and the aux region
INSIDE one mipx_execute_dev workspace are not fenced from each other (the per-op cases
cover each kernel's own footprint, the plan cases the workspace's outer bounds).
"""
import pytest

FILL = 0xA5


@pytest.fixture(autouse=True)
def guarded():
    from imaginary_amd import engine
    prev = engine.set_guard(FILL, 0, 0)
    yield
    engine.set_guard(*prev)
