"""Where each set of weights lies while another stands in flat_w (ursonet_amd/train_state.py): the whole table of
weights_location as literals -- four sets x four stand-ins, and the one cell that depends on Config.WEIGHT_EMA."""
import os
import subprocess
import sys

import pytest

from ursonet_amd.train_state import SETS, STAND_INS, weights_location

#            stand_in:  None           "ema"          "swa"          "swag"
TABLE = {
    "raw": ("flat_w", "flat_ema", "flat_swa", "flat_w"),
    "ema": ("flat_ema", "flat_w", "flat_ema", "flat_ema"),
    "swa": ("flat_swa", "flat_swa", "flat_w", "flat_swa"),
    "sq": ("flat_swa_sq", "flat_swa_sq", "flat_swa_sq", "flat_swa_sq"),
}


def test_the_table_names_every_set_and_every_stand_in():
    assert STAND_INS == (None, "ema", "swa", "swag") and SETS == ("raw", "ema", "swa", "sq") and set(TABLE) == set(SETS)


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("col,stand_in", list(enumerate(STAND_INS)), ids=lambda v: str(v))
def test_weights_location_cell(which, col, stand_in):
    assert weights_location(stand_in, which, True) == TABLE[which][col]
    assert weights_location(stand_in, which) == TABLE[which][col]                  # has_ema defaults to True


def test_raw_weights_without_an_ema_buffer_are_wviews_default():
    """No Config.WEIGHT_EMA and nothing stands in: None, which Engine.wview reads as flat_w.  Every other cell an engine without the
    average can reach ("ema" never stands in there) is the table's."""
    assert weights_location(None, "raw", False) is None
    for col, stand_in in enumerate(STAND_INS):
        for which in ("swa", "sq") + (("raw",) if stand_in in ("swa", "swag") else ()):
            assert weights_location(stand_in, which, False) == TABLE[which][col], (stand_in, which)


def test_each_set_lies_in_one_buffer_and_each_buffer_holds_one_set():
    """Under every stand-in the three exchangeable sets lie in three different buffers, flat_w among them."""
    for stand_in in STAND_INS:
        where = [weights_location(stand_in, w) for w in ("raw", "ema", "swa")]
        assert len(set(where)) == 3 and "flat_w" in where, (stand_in, where)


def test_unknown_names_are_refused():
    with pytest.raises(AssertionError):
        weights_location("sq", "raw")
    with pytest.raises(AssertionError):
        weights_location(None, "swag")


def test_module_imports_neither_torch_nor_the_engine():
    code = ("import sys; import ursonet_amd.train_state; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules "
            "and 'ursonet_amd.engine' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
