"""Where each set of weights lies while another one stands in flat_w.  Host arithmetic on names alone: no torch, no
engine, so the table can be enumerated without a GPU (tests/test_train_state_cpu.py).

The Engine keeps up to four sets: the raw weights, the EMA average (flat_ema), the SWA mean (flat_swa) and SWA's mean of squares
(flat_swa_sq).  Every forward pass reads flat_w, so an average becomes the model by changing places with the raw weights (swap_ema /
swap_swa), and a SWAG sample by overwriting them while they wait in a hold buffer.  Engine._stand_in names which of these holds now."""

STAND_INS = (None, "ema", "swa", "swag")
SETS = ("raw", "ema", "swa", "sq")


def weights_location(stand_in, which, has_ema=True):
    """The Engine attribute that holds the set `which` while `stand_in` stands in flat_w; None = flat_w by Engine.wview's default (an engine
    without Config.WEIGHT_EMA that nothing stands in for).  Under "swag" the raw set is the sample: it is the model then."""
    assert stand_in in STAND_INS and which in SETS, (stand_in, which)
    if which == "sq":                                  # never exchanged
        return "flat_swa_sq"
    if which == stand_in:                              # the set that changed places with the raw weights
        return "flat_w"
    if which != "raw":                                 # an average at home
        return "flat_" + which
    if stand_in in ("ema", "swa"):                     # the raw weights wait in the buffer of the average that stands in
        return "flat_" + stand_in
    return "flat_w" if has_ema or stand_in else None
