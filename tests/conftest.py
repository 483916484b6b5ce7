import gzip
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Index range checks on every kernel launch in tests (host sync per op: fine here).
os.environ.setdefault("FM_DEBUG_CHECKS", "1")

# The reference's sample.cfg and heads of its sample data set (tests/golden/README.md).
GOLDEN_REF = os.path.join(ROOT, "tests", "golden", "reference")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU; run with -m gpu")
    config.addinivalue_line("markers", "slow: long-running test")


def _gpu_available() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


def pytest_collection_modifyitems(config, items):
    if _gpu_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def ref_sample_dir(tmp_path_factory):
    """The reference's sample.cfg next to its data/ files, unpacked from tests/golden/reference."""
    d = tmp_path_factory.mktemp("reference")
    shutil.copy(os.path.join(GOLDEN_REF, "sample.cfg"), d / "sample.cfg")
    (d / "data").mkdir()
    for name in sorted(os.listdir(os.path.join(GOLDEN_REF, "data"))):
        assert name.endswith(".gz"), name
        with gzip.open(os.path.join(GOLDEN_REF, "data", name), "rb") as f, open(d / "data" / name[:-3], "wb") as g:
            shutil.copyfileobj(f, g)
    return str(d)


@pytest.fixture(scope="session")
def ref_data_dir(ref_sample_dir):
    return os.path.join(ref_sample_dir, "data")
