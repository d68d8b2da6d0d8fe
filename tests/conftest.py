import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The resident apply needs GPU_MAX_HW_QUEUES >= 8 (include/blinky_hip.h, bk_set_resident_share): with fewer hardware queues a
# stream shares one with a resident kernel and waits for its idle exit, so tests that run several stripe contexts' resident
# kernels on one GPU would see them restart every frame.  libblinkyhip raises the variable only when it is unset and only when
# it is loaded before the HIP runtime; the suite sets it here, before any test starts the runtime, when the environment
# leaves it lower.
_hwq = os.environ.get("GPU_MAX_HW_QUEUES", "")
if not _hwq.isdigit() or int(_hwq) < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "ref: needs oracle/_ref (built from /root/reference in the build container)")


@pytest.fixture(scope="session", autouse=True)
def _built():
    """Make sure the oracle (checker) and the HIP library (product) are built.
    Building the checker is not using it; the GPU box normally receives prebuilt files."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "liboracle.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle.so", "liboracle_bkm.so"])
    if not os.path.exists(os.path.join(ROOT, "blinky_amd", "libblinkyhip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "blinky_amd", "csrc")])
    yield
