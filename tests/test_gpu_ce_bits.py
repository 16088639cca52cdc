"""The four older cross-entropy entries and qarig_token_score write, buffer for buffer, the bits they wrote before the
loss path was folded into one row kernel, one mean kernel and one launcher: tools/ce_bits.py recomputes
its SHA-256 digests -- loss, row_ws, the whole dlogits buffer with its pad, row_nll, row_rank, the flag -- and every one
must equal tests/golden/ce_parent_bits.json, recorded by the same tool on the commit named in that file.  The build
has -ffp-contract=off: a digest that differs is an operation that changed."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def test_every_digest_of_the_parent_commit():
    import ce_bits
    with open(os.path.join(ROOT, "tests", "golden", "ce_parent_bits.json")) as f:
        want = json.load(f)["digests"]
    got = ce_bits.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == 141 and {k.split()[0] for k in want} == {"plain", "ld", "reg", "soft", "score"}
    differ = [(k, b) for k in want for b in want[k] if got[k].get(b) != want[k][b]]
    assert not differ, differ
    assert all(sorted(got[k]) == sorted(want[k]) for k in want)
