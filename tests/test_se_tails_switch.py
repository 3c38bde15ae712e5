"""lss_se_tails (include/lss_convs.h): the switch returns the previous setting; no GPU needed."""
import os

from lss_carla_amd import _lib


def test_lss_se_tails_returns_previous_and_restores():
    lib = _lib.load()
    first = lib.lss_se_tails(0)
    try:
        assert first in (0, 1, 2)
        if not os.environ.get("LSS_LIB"):  # the product library starts with the tails on
            assert first == 1
        assert lib.lss_se_tails(1) == 0
        assert lib.lss_se_tails(2) == 1
        assert lib.lss_se_tails(7) == 2   # 2 and above: on for every shape
        assert lib.lss_se_tails(-3) == 2
        assert lib.lss_se_tails(0) == 0   # zero and below: off
    finally:
        lib.lss_se_tails(first)
    assert lib.lss_se_tails(first) == first
