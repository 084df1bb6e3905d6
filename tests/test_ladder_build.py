"""The feature ladder ("The feature ladder"), what can be checked on the source text without a GPU: the rungs' launchers are
reached through ONE table (csrc/rmav_ladder.hpp) and from nowhere else; the rung units no longer carry launchers of their own; the
precedence of the handle's switches is written once, in rung_of, and the table is indexed with nothing else; the kernel headers set their
guards through the two fragments; the build still has its sixteen units."""
import glob
import os
import re

import buildinfo as B

CSRC = os.path.join(B.PKG, "csrc")
# rung -> (the unit's name in rmav_launch_<x>_*, its unit, its policy unit or None), in ladder order
RUNGS = [("ranged", "rmav_range_abi", None), ("skip", "rmav_skip_abi", None), ("reward", "rmav_reward_abi", None), ("disturb", "rmav_disturb_abi", None),
         ("sensor", "rmav_sensor_abi", "rmav_sensor_policy_abi"), ("actuator", "rmav_actuator_abi", "rmav_actuator_policy_abi"),
         ("start", "rmav_start_abi", "rmav_start_policy_abi"), ("term", "rmav_term_abi", "rmav_term_policy_abi")]
SWITCHES = ("term_on", "start_on", "actuator_on", "sensor_on", "disturb_on")
UNITS = ["rmav_abi", "rmav_ppo_abi", "rmav_comm_abi", "rmav_range_abi", "rmav_skip_abi", "rmav_reward_abi", "rmav_disturb_abi", "rmav_sensor_abi",
         "rmav_actuator_abi", "rmav_start_abi", "rmav_term_abi", "rmav_policy_abi", "rmav_sensor_policy_abi", "rmav_actuator_policy_abi",
         "rmav_start_policy_abi", "rmav_term_policy_abi"]


def code(name):
    """a source of csrc/ without its comments"""
    txt = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def sources():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".hip", ".hpp", ".inc")))


def functions(name):
    """{function name: text} of the top-level function definitions of a source: a definition starts in column 0 (its signature may run
    over several lines), its body opens with the first line that ends with '{' and closes with the next '}' in column 0"""
    out, head, cur, body = {}, [], None, []
    for ln in code(name).split("\n"):
        if cur is not None:
            body.append(ln)
            if ln.startswith("}"):
                out[cur] = out.get(cur, "") + "\n".join(body)
                cur = None
        elif head or (re.match(r"[A-Za-z_]", ln) and not ln.startswith(("namespace", "struct", "enum", "extern", "using", "constexpr", "typedef"))):
            head.append(ln)
            if ln.rstrip().endswith("{"):
                m = re.search(r"(\w+)\s*\(", re.sub(r"__attribute__\(\(.*?\)\)|__launch_bounds__\(.*?\)\s", "", " ".join(head)))
                cur, body, head = (m.group(1) if m else None), list(head), []
            elif ln.rstrip().endswith((";", "}")):
                head = []
    return out


def test_every_rung_launcher_is_reached_through_the_table_alone():
    table = code("rmav_ladder.hpp")
    rows = table[table.index("constexpr RungRow kLadder[RUNG_COUNT]"):]
    for x, unit, policy in RUNGS:
        for fn, home in ((f"rmav_launch_{x}_rollout", unit), (f"rmav_launch_{x}_step", unit), (f"rmav_launch_{x}_policy_rollout", policy)):
            if home is None:
                assert not any(fn in code(f) for f in sources()), fn
                continue
            where = {f: len(re.findall(r"\b" + fn + r"\b", code(f))) for f in sources()}
            where = {f: c for f, c in where.items() if c}
            assert where == {home + ".hip": 1, "rmav_handle.hpp": 1, "rmav_ladder.hpp": 1}, (fn, where)
            assert re.search(r"\bint " + fn + r"\(", code("rmav_handle.hpp")), f"{fn}: the declaration"
            assert re.search(r"\b" + fn + r"\b", rows), f"{fn}: the table row"
    # the rows stand in ladder order, one per rung, behind the row of a handle that is on no rung
    assert re.findall(r"\brmav_launch_(\w+?)_step\b", rows) == [x for x, _, _ in RUNGS]
    enum = re.search(r"enum Rung : int \{([^}]*)\}", table).group(1).replace(" ", "").split(",")
    assert enum == ["RUNG_NONE=0", "RUNG_RANGE", "RUNG_SKIP", "RUNG_REWARD", "RUNG_DISTURB", "RUNG_SENSOR", "RUNG_ACTUATOR", "RUNG_START", "RUNG_TERM", "RUNG_COUNT"]
    # a row's two phrases stay in step: `who` is `handle`, or `handle` and the setter's name in brackets
    phrases = re.findall(r'\{"([^"]+)", "([^"]+)", "([^"]+)", rmav_launch_', rows)
    assert len(phrases) == len(RUNGS), phrases
    for noun, handle, who in phrases:
        assert who == handle or re.fullmatch(re.escape(handle) + r" \(rmav_set_\w+\)", who), (noun, handle, who)
    # no std::function, nothing virtual, no allocation in the table's header
    for word in ("std::function", "virtual", "new ", "malloc"):
        assert word not in table, word


def test_the_rung_units_carry_no_launcher_of_their_own():
    for f in sources():
        if not f.endswith("_abi.hip"):
            continue
        src = code(f)
        assert not re.search(r"\blaunch_km\b", src) and not re.search(r"\bdispatch_reward\b", src), f
    for x, unit, policy in RUNGS:
        src = code(unit + ".hip")
        assert '#include "rmav_rung_launch.hpp"' in src and not re.search(r"hipLaunchKernelGGL\(\(?k_(rollout|step)", src) and "tl_args" not in src, unit
        assert src.count("launch_rung_rollout<") == 1 and src.count("launch_rung_step<") == 1, unit
        if policy:
            src = code(policy + ".hip")
            assert '#include "rmav_policy_rung.hpp"' in src and src.count("launch_policy_rung<") == 1, policy
            for word in ("take_armed_exchange", "check_rollout_launch", "pair_group", "kNormBytes", "struct Shape"):
                assert word not in src, (policy, word)
    # the argument list of every rung is built in one function
    assert sum("rung_tail(" in code(f) and "auto rung_tail(" in code(f) for f in sources()) == 1
    users = [f for f in sources() if re.search(r"\b(start_actuator_args|term_start_args|disturb_or_calm)\(h", code(f)) and f != "rmav_handle.hpp"]
    assert users == ["rmav_rung_launch.hpp"], users


def test_the_precedence_of_the_switches_is_written_once():
    ladder = functions("rmav_ladder.hpp")
    assert "rung_of" in ladder
    tests = re.findall(r"if \(h->(\w+)(?: > 1)?\) return (RUNG_\w+);", ladder["rung_of"])
    assert tests == [("term_on", "RUNG_TERM"), ("start_on", "RUNG_START"), ("actuator_on", "RUNG_ACTUATOR"), ("sensor_on", "RUNG_SENSOR"),
                     ("disturb_on", "RUNG_DISTURB"), ("reward_on", "RUNG_REWARD"), ("frame_skip", "RUNG_SKIP"), ("range_mask", "RUNG_RANGE")], tests
    # routing = choosing a rung's launcher: the table is the only way to one (the test above), and it is indexed with rung_of(h), with a
    # variable that holds rung_of(h), or with a rung's own constant - in the routing sources and in the launchers' headers
    for f in sources():
        src = code(f)
        for idx in re.findall(r"kLadder\[([^\]]*)\]", src):
            assert idx in ("r", "R", "rung_of(h)", "RUNG_RANGE", "RUNG_COUNT"), (f, idx)
        for init in re.findall(r"\bRung r\b\s*=\s*(\w+\([^()]*\))", src):
            assert init == "rung_of(h)", (f, init)
        assert len(re.findall(r"\bRung r\b\s*=", src)) == len(re.findall(r"\bRung r\b\s*=\s*rung_of\(h\)", src)), f
    # ... and outside rung_of no function of the host sources compares the switches with one another: none reads two of them but the
    # setters, getters and reset paths, which act on their own feature (the argument providers of rmav_handle.hpp are not routing)
    own = re.compile(r"^(rmav_(set|get)_\w+|rmav_reset|rmav_observe|launch_reset\w*|rmav_disturbance_now|rmav_(get|set)_actuator_state)$")
    for f in sources():
        if not f.endswith(".hip"):
            continue
        for fn, body in functions(f).items():
            read = {s for s in SWITCHES if re.search(r"h->" + s + r"\b(?!\s*=[^=])", body)}
            assert len(read) <= 1 or own.match(fn), (f, fn, sorted(read))


def test_the_kernel_headers_set_their_guards_through_the_fragments():
    for hdr, prefix, frag, stacks in (("rmav_kernels.hpp", "RMAV_ROLLOUT_", "rmav_rollout_rung.inc", 8), ("rmav_policy_pair.hpp", "RMAV_PAIR_", "rmav_pair_rung.inc", 16)):
        txt = open(os.path.join(CSRC, hdr)).read()
        assert not re.search(r"#define " + prefix + r"\w+ 1", txt), hdr
        assert not re.search(r"#undef " + prefix, txt), hdr
        assert len(re.findall(r'^#define RMAV_RUNG \d\n(?:#define RMAV_PAIR_BODY "rmav_pair(?:_shared)?_body\.inc"\n)?#include "' + re.escape(frag) + '"$', txt, flags=re.M)) == stacks, hdr
        f = open(os.path.join(CSRC, frag)).read()
        guards = sorted(set(re.findall(r"#define (" + prefix + r"[A-Z]+) 0", txt)))
        assert len(guards) == (4 if prefix == "RMAV_ROLLOUT_" else 6), (hdr, guards)
        for g in guards:   # set from the number in front of the body, back to 0 behind it
            on, off = f.index(f"#define {g} (RMAV_RUNG >= "), f.index(f"#define {g} 0")
            assert on < f.index("#include ") < off, (frag, g)
        assert f.rstrip().endswith("#undef RMAV_PAIR_BODY" if prefix == "RMAV_PAIR_" else "#undef RMAV_RUNG") and "#undef RMAV_RUNG" in f, frag
    # a kernel's suffix is its rung's number
    number = {"dr": 1, "fs": 2, "rw": 3, "ds": 4, "sn": 5, "al": 6, "ss": 7, "tc": 8}
    for hdr in ("rmav_kernels.hpp", "rmav_policy_pair.hpp"):
        txt = open(os.path.join(CSRC, hdr)).read()
        seen = re.findall(r"void k_rollout_(?:nrm_|pair_shared_|pair_)?([a-z]{2})\((?:(?!\nvoid |\n\}\n).)*?#define RMAV_RUNG (\d)", txt, flags=re.S)
        assert seen and all(number[sfx] == int(n) for sfx, n in seen), (hdr, seen)


def test_the_build_still_has_its_sixteen_units():
    mk = open(os.path.join(B.PKG, "Makefile")).read()
    units = re.search(r"^ABI_UNITS\s*:=(.*)$", mk, re.M).group(1).split() + re.search(r"^POLICY_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert units == UNITS
    assert sorted(f[:-4] for f in sources() if f.endswith(".hip")) == sorted(UNITS)
