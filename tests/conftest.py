import os
import pty

import pytest


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test requires an MI355X GPU")


@pytest.fixture
def pty_device():
    """Skip on a host that cannot allocate a pseudo-terminal (no
    /dev/ptmx or devpts, as in some sandboxes); attachable shims need one."""
    try:
        master, slave = pty.openpty()
    except OSError as e:
        pytest.skip(f"needs a PTY device, host has none: {e}")
    os.close(master)
    os.close(slave)
