import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")



def _miopen_dirs(repo: str) -> tuple:
    """bench.miopen_dirs, restated (bench.py stays one file and imports torch; this must run before
    torch starts): a working copy of the committed MIOpen databases under the git-ignored cache
    directory, or under a per-user temporary directory where the tree cannot be written."""
    import hashlib
    import shutil
    import tempfile
    src = os.path.join(repo, "tuning", "miopen", "db")
    in_tree = os.path.join(repo, "tuning", "miopen", "cache")
    tag = hashlib.sha1(os.path.abspath(repo).encode()).hexdigest()[:10]
    for cache in (in_tree, os.path.join(tempfile.gettempdir(), f"lss_miopen_{os.getuid()}_{tag}")):
        db = os.path.join(cache, "db")
        try:
            os.makedirs(db, mode=0o700, exist_ok=True)
            if not os.access(db, os.W_OK):
                raise PermissionError(db)
            for name in os.listdir(src):
                s, d = os.path.join(src, name), os.path.join(db, name)
                if not os.path.exists(d) or os.path.getmtime(s) > os.path.getmtime(d):
                    tmp = f"{d}.{os.getpid()}.tmp"
                    shutil.copyfile(s, tmp)
                    os.replace(tmp, d)
            return db, cache
        except OSError:
            continue
    return src, in_tree


# MIOpen find results kept in-tree (as bench.py uses them): the conv tests skip the exhaustive search
if "MIOPEN_USER_DB_PATH" not in os.environ or "MIOPEN_CUSTOM_CACHE_DIR" not in os.environ:
    _db, _cache = _miopen_dirs(REPO)
    os.environ.setdefault("MIOPEN_USER_DB_PATH", _db)
    os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", _cache)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through the HIP C-ABI library)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


def gpu_available() -> bool:
    import torch
    return torch.cuda.is_available()


@pytest.fixture(autouse=True)
def _lss_debug_checks(request):
    """LSS_DEBUG=1 (liblss_hip_debug.so): after every GPU test, no device-side index check may have
    failed (include/lss_hip.h, lss_debug_status)."""
    yield
    if os.environ.get("LSS_DEBUG", "0") != "1" or request.node.get_closest_marker("gpu") is None:
        return
    import torch
    if not torch.cuda.is_available():
        return
    from lss_carla_amd import _lib
    torch.cuda.synchronize()
    st = _lib.debug_status(clear=True)
    assert _lib.load().lss_debug_checks() == 1, "LSS_DEBUG=1 but the product library was loaded"
    assert st[0] == 0, f"device index check failed: {st[0]} failures, first: code {st[1]} value {st[2]} bound {st[3]}"
