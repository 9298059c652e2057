"""The sample bounds of a field's train state (`render.TrainState`) through a fixed script of events.  The deterministic mode's partial-sum
grouping depends on these exact bounds, so the expected values are literals: they were produced once by the dict-based `_grow_caps` / `_caps_for`
this class replaced, run on the same script.  No GPU and no library load."""
from apnrf_amd import render as RD

# ("caps", R, expected (max_marched, max_kept)) | ("grow", marched, kept, R, carry) | ("reserve", max_marched, max_kept)
SCRIPT = [
    # a fresh state: R * 384 crosses the 1 << 18 floor of the marched bound between 682 and 683 rays
    ("caps", 16, (262144, 3072)),
    ("caps", 500, (262144, 96000)),
    ("caps", 682, (262144, 130944)),
    ("caps", 683, (262272, 131136)),
    ("caps", 2000, (768000, 384000)),
    ("caps", 8192, (3145728, 1572864)),
    # a synchronous overflow (carry=False) raises the bounds of its own ray count only; they never shrink; kept < marched // 2 takes the marched form
    ("grow", 1500000, 400000, 2000, False),
    ("caps", 2000, (1951024, 976024)),
    ("caps", 4096, (1572864, 786432)),
    ("caps", 16, (262144, 3072)),
    ("grow", 900000, 1000000, 2000, False),
    ("caps", 2000, (1951024, 1301024)),
    ("caps", 1999, (767616, 383808)),
    ("grow", 300000, 10, 16, False),
    ("caps", 16, (391024, 196024)),
    ("caps", 2000, (1951024, 1301024)),
    # an asynchronous overflow (carry=True) raises an absolute and a per-ray bound: smaller ray counts get the first, larger ones the second
    ("grow", 2000000, 100000, 1000, True),
    ("caps", 100, (2601024, 1301024)),
    ("caps", 1000, (2601024, 1301024)),
    ("caps", 2000, (5202048, 2602048)),
    ("caps", 16, (2601024, 1301024)),
    ("caps", 50000, (130051200, 65051199)),
    ("grow", 700001, 650000, 333, True),
    ("caps", 100, (2601024, 1301024)),
    ("caps", 333, (2601024, 1301024)),
    ("caps", 50000, (136790540, 127030630)),
    # reserve, then growth below and above the reserved bound
    ("reserve", 3145728, 1048576),
    ("caps", 16, (3145728, 1301024)),
    ("caps", 2000, (5471621, 5081225)),
    ("caps", 50000, (136790540, 127030630)),
    ("grow", 1000000, 200000, 4096, True),
    ("caps", 16, (3145728, 1301024)),
    ("caps", 4096, (11205881, 10406349)),
    ("caps", 50000, (136790540, 127030630)),
    ("grow", 5000000, 3000000, 4096, True),
    ("caps", 16, (6501024, 3901024)),
    ("caps", 2000, (6501024, 5081225)),
    ("caps", 4096, (11205881, 10406349)),
    ("caps", 50000, (136790540, 127030630)),
    ("reserve", 1048576, 524288),
    ("caps", 2000, (6501024, 5081225)),
]


def test_bounds_follow_the_script_exactly():
    st = RD.TrainState()
    for n, (what, *args) in enumerate(SCRIPT):
        if what == "caps":
            assert st.caps(args[0]) == args[1], (n, args)
        else:
            getattr(st, what)(*args)


def test_a_fresh_state_declares_every_field():
    st = RD.TrainState()
    assert vars(st) == dict(by_R={}, abs_m=0, abs_k=0, per_m=0.0, per_k=0.0, pending=[], pinned=[], last_counts=None, skipped_steps=0,
                            sched_debt=0, overflowed_steps=0)


def test_step_verdict_reads_the_status_word():
    import pytest
    assert RD._step_verdict(10, 5, 3, 0, 0) == RD._STEP_OK and RD._step_verdict(0, 0, 0, RD._ST_EMPTY, 1) == RD._STEP_OK
    assert RD._step_verdict(10, 5, 3, RD._ST_MARCHED, 1) == RD._STEP_GROW and RD._step_verdict(10, 5, 3, RD._ST_KEPT, 1) == RD._STEP_GROW
    assert RD._step_verdict(10, 5, 3, RD._ST_ROW | RD._ST_KEPT, 1) == RD._STEP_ROW
    with pytest.raises(RD.L.MnfError, match="class id"):
        RD._step_verdict(10, 5, 3, RD._ST_LABEL | RD._ST_ROW, 1)
