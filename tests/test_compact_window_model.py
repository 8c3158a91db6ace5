"""The windowed compaction model (tests/compact_window_ref.py: carried tables, mark bytes, rescan, FIFO carry) against the whole-list
rule (tests/compact_ref.py) on the shared corpus: whole, op by op, at random cuts, with scan cuts that differ from the feed cuts,
and with the rewrite pass rewound and repeated.  No GPU."""
import numpy as np
import pytest

import compact_cases
import compact_ref
import compact_window_ref as cw
from reverie_amd.ops import DOM_B2A

CORPUS = compact_cases.corpus() + [("of_length_%d" % n, *compact_cases.of_length(n, n)) for n in range(3000, 3006)]
ERRORS = compact_cases.error_cases()


def _random_cuts(rng, n, k):
    return sorted(rng.integers(0, n + 1, k).tolist()) if n else [0] * k


@pytest.mark.parametrize("name,prog,wc", CORPUS, ids=[c[0] for c in CORPUS])
def test_model_equals_the_rule(name, prog, wc):
    rc, want, counts, info = compact_ref.compact(prog, wc)
    assert rc == 0
    n = len(prog)
    rng = np.random.default_rng(n)
    ways = [((), ()), (_random_cuts(rng, n, 5), _random_cuts(rng, n, 7)), (_random_cuts(rng, n, 3), ())]
    if n <= 3000:
        ways.append((range(1, n), range(1, n)))
    for scan_cuts, feed_cuts in ways:
        rc, outs, c2, i2, scans = cw.compact_windowed(prog, wc, scan_cuts, feed_cuts, passes=2)
        assert rc == 0 and c2 == counts and i2 == info
        assert scans == (2 if (prog["domain"] == DOM_B2A).any() else 1)
        for out in outs:  # (the second one after a rewind)
            assert out.tobytes() == want.tobytes()


@pytest.mark.parametrize("name,prog,wc,code", ERRORS, ids=[e[0] for e in ERRORS])
def test_model_error_codes(name, prog, wc, code):
    want = compact_ref.compact(prog, wc)[0]
    assert want != 0 and (code is None or code == want)
    for cuts in ((), range(1, len(prog))):
        assert cw.compact_windowed(prog, wc, cuts)[0] == want


def test_model_order_of_calls():
    prog, wc = compact_cases.chain(10)
    c = cw.WindowCompactor(wc)
    assert c.feed(prog)[0] == cw.E_ARG and c.rewind() == cw.E_ARG
    assert c.scan(prog) == 0 and c.scan_end() == (0, 0)
    assert c.scan(prog) == cw.E_ARG and c.rewind() == cw.E_ARG  # (a short pass is not rewound)
    assert c.feed(prog[:5])[0] == 0 and c.feed(prog)[0] == cw.E_ARG
    assert c.feed(prog[5:])[0] == 0 and c.rewind() == 0
