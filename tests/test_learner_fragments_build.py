"""The fused learners share their tile walk and loss terms as text (csrc/rmav_learner_*.inc), what can be checked without a GPU: each
fragment is included exactly once by each of the two learner headers and by nothing else, and the arithmetic and the host check that
used to be typed twice stand in one file of csrc/ each."""
import glob
import os
import re

import buildinfo as B

CSRC = os.path.join(B.PKG, "csrc")
HEADERS = ("rmav_learner.hpp", "rmav_learner_shared.hpp")
FRAGMENTS = ("rmav_learner_bwd.inc", "rmav_learner_fwd.inc", "rmav_learner_pg.inc", "rmav_learner_stage.inc", "rmav_learner_vf.inc")


def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p)}


def test_each_fragment_is_included_once_by_each_header_and_by_nothing_else():
    src = _sources()
    assert tuple(sorted(f for f in src if re.fullmatch(r"rmav_learner_.*\.inc", f))) == FRAGMENTS
    for frag in FRAGMENTS:
        count = {f: len(re.findall(r'^\s*#\s*include\s+"' + re.escape(frag) + '"', txt, flags=re.M)) for f, txt in src.items()}
        assert {f: c for f, c in count.items() if c} == {h: 1 for h in HEADERS}, (frag, count)


def test_the_shared_arithmetic_and_the_host_check_stand_once():
    src = _sources()
    for literal in ("1.8378770664093453f", "fmaxf(e1, e2)", "batch must be in [1, 2^31)"):
        where = [f for f, txt in src.items() if literal in txt]
        assert len(where) == 1, (literal, where)
        assert sum(txt.count(literal) for txt in src.values()) == 1, literal
