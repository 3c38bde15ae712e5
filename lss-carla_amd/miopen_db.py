"""The committed MIOpen find results (tuning/miopen/db: which conv solver per shape) for this process.

``bench.py`` and the test suite point MIOpen at a working copy of those databases before torch starts;
without them MIOpen picks its default solvers and the config-3 step is ~2 ms slower (measured: 12.5 ms
against 10.6 ms). ``use_committed()`` does the same for any entry point of the package -- the trainer calls
it when it is imported. It only sets ``MIOPEN_USER_DB_PATH`` / ``MIOPEN_CUSTOM_CACHE_DIR`` where the
caller has not, and must run before the first convolution (best: before ``import torch``). No torch import
here.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dirs(repo: str = REPO) -> tuple:
    """(user db, kernel cache): MIOpen rewrites its user databases while it runs, so it gets a working
    copy of the committed ones under the git-ignored cache directory (refreshed when a committed file is
    newer), or under a per-user temporary directory where the tree cannot be written."""
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
                    tmp = f"{d}.{os.getpid()}.tmp"  # (several processes may start at once: the copy appears whole)
                    shutil.copyfile(s, tmp)
                    os.replace(tmp, d)
            return db, cache
        except OSError:
            continue
    return src, in_tree


def use_committed() -> None:
    if "MIOPEN_USER_DB_PATH" in os.environ and "MIOPEN_CUSTOM_CACHE_DIR" in os.environ:
        return
    if not os.path.isdir(os.path.join(REPO, "tuning", "miopen", "db")):
        return
    db, cache = dirs()
    os.environ.setdefault("MIOPEN_USER_DB_PATH", db)
    os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", cache)
