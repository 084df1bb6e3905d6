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


def test_every_fragment_resolves_and_is_shared():
    """The kernel bodies are shared as text: every #include "….inc" names a file of csrc/, and a fragment that another
    .inc includes has at least two users - one with a single user shares nothing and belongs back in the file that includes it."""
    users = {}
    sources = sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".hip", ".hpp", ".inc")))
    for p in sources:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+\.inc)"', _code(p), flags=re.M):
            assert os.path.isfile(os.path.join(CSRC, inc)), f"{os.path.basename(p)} includes {inc}, which is not in csrc/"
            users.setdefault(inc, []).append(os.path.basename(p))
    assert users, "no .inc is included at all: the pattern above no longer matches the sources"
    on_disk = sorted(os.path.basename(p) for p in sources if p.endswith(".inc"))
    assert sorted(users) == on_disk, f"never included: {sorted(set(on_disk) - set(users))}"
    nested = {inc: who for inc, who in users.items() if any(w.endswith(".inc") for w in who)}
    assert nested, "the pair bodies and the one-wavefront body share their common statements as nested fragments"
    for inc, who in sorted(nested.items()):
        assert len(who) >= 2, f"{inc} is included once, from {who[0]}: inline it back"


def test_no_undeclared_entry_point():
    declared = set().union(*(_declared(h) for h in PAIRS))
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        extra = sorted(set(_defined(p)) - declared)
        assert not extra, f"{os.path.basename(p)} defines {extra} inside extern \"C\" without a declaration in include/"
