"""The host side of the C ABI is one source per public header (source text only: no build, no GPU): every function a header declares
is defined in the .hip file paired with it and in no other, and no .hip file defines an extern "C" rmav_* function without a
declaration."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reinmav-gym_amd", "csrc")
PAIRS = {"rmav.h": "rmav_abi.hip", "rmav_ppo.h": "rmav_ppo_abi.hip", "rmav_comm.h": "rmav_comm_abi.hip"}


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def _declared(header):
    return set(re.findall(r"\b(rmav_[a-z0-9_]+)\s*\(", _code(os.path.join(ROOT, "include", header))))


def _defined(path):
    """the rmav_* functions the extern "C" block of a .hip file defines: a definition starts a line with its return type (a call or a
    static helper does not) and its parameter list is followed by a brace"""
    code = _code(path)
    if 'extern "C" {' not in code:
        return []
    body = code[code.index('extern "C" {'):]
    return re.findall(r"^(?:const char \*|int64_t |int )(rmav_[a-z0-9_]+)\s*\([^;{}]*\)\s*\{", body, flags=re.M)


def test_every_header_is_implemented_by_its_own_source():
    defined = {os.path.basename(p): _defined(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}
    assert set(PAIRS.values()) <= set(defined)
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(PAIRS)
    for header, source in PAIRS.items():
        names = _declared(header)
        assert len(names) >= 10, (header, len(names))
        for n in sorted(names):
            where = [f for f, d in defined.items() if n in d]
            assert where == [source], f"{n} is declared in include/{header}: it belongs in csrc/{source} alone, found in {where}"
            assert defined[source].count(n) == 1, n


def test_no_undeclared_entry_point():
    declared = set().union(*(_declared(h) for h in PAIRS))
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        extra = sorted(set(_defined(p)) - declared)
        assert not extra, f"{os.path.basename(p)} defines {extra} inside extern \"C\" without a declaration in include/"
