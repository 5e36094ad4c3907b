"""The Python mirrors of the C ABI (spec/layout.py: kbj_model, kbj_config, the record-offset tables, the constants; host/binding.py: nine
more structs and the prototypes of every entry point) against include/kbj.h as the host compiler reads it (tests/abi_probe.py): every
field's offset, size and type, every enumerator's value, every constant, every prototype's arity and argument types, by name. The header
text itself is read for NAMES only: that it defines no struct, enumerator or function without a mirror. The checks are functions that
return what they object to, so that the last test can hand them mutated copies of the mirrors - among them the three that the former
checks (sizeof equality, name-set equality) let through. Needs g++, no GPU and no library."""
import ctypes as C
import os
import re

import pytest

from kbot_joystick_amd.host import binding as B
from kbot_joystick_amd.spec import constants, layout as L
from tests import abi_probe as P

HEADERS = ("kbj_model.h", "kbj.h")
f32, i32 = C.c_float, C.c_int32


@pytest.fixture(scope="module")
def rep(tmp_path_factory):
    return P.report(tmp_path_factory.mktemp("abi_probe"))


@pytest.fixture(scope="module")
def text():
    """The two headers without their comments."""
    raw = "\n".join(open(os.path.join(P.INCLUDE, h)).read() for h in HEADERS)
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", raw, flags=re.S)


# ---- the checks: each returns the list of its objections, every one starting with the struct, table or function it is about ----
def struct_errors(rep, cname, cls):
    errs = []
    if rep.sizeof[cname] != C.sizeof(cls):
        errs.append(f"{cname}: sizeof is {rep.sizeof[cname]} in the header, {C.sizeof(cls)} in {cls.__name__}")
    for name, *got in P.ctypes_fields(cls):
        want = rep.fields[cname].get(name)
        if want != tuple(got):
            errs.append(f"{cname}.{name}: (offset, size, kind) is {want} in the header, {tuple(got)} in {cls.__name__}")
    return errs


def table_errors(rep, name, table):
    return [f"{name}: {key} is {rep.enums.get(f'KBJ_{name}_{key}')} in the header, {value} in layout.{name}"
            for key, value in table.items() if rep.enums.get(f"KBJ_{name}_{key}") != value]


def signature_errors(rep, name, sig):
    want, got = rep.prototypes[name], P.ctypes_signature(sig)
    if want == got:
        return []
    (wr, wa), (gr, ga) = want.split(":"), got.split(":")
    errs = [f"{name}: returns {wr} in the header, {gr} in SIGNATURES"] if wr != gr else []
    if len(wa) != len(ga):
        errs.append(f"{name}: takes {len(wa)} arguments ({wa}) in the header, {len(ga)} ({ga}) in SIGNATURES")
    errs += [f"{name}: argument {k} is {a} in the header, {b} in SIGNATURES" for k, (a, b) in enumerate(zip(wa, ga)) if a != b]
    return errs


def header_structs(text):
    return set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", text))


def header_functions(text):
    return set(re.findall(r"\b(kbj_[a-z0-9_]+)\s*\(", text))


def header_enumerators(text):
    """The identifier of every enumerator of every enum body, with or without an initialiser."""
    items = [item for body in re.findall(r"\benum\b[^{;]*\{(.*?)\}", text, re.S) for item in body.split(",")]
    return [m.group(1) for m in (re.match(r"\s*([A-Za-z_]\w*)", item) for item in items) if m]


def enumerator_errors(text, tables):
    """Every enumerator of the header belongs, by the longest prefix KBJ_<table>_, to one mirrored table, which has its key."""
    errs = []
    for e in header_enumerators(text):
        owners = [n for n in tables if e.startswith(f"KBJ_{n}_")]
        if not owners:
            errs.append(f"{e}: belongs to no table that layout.py mirrors")
            continue
        name = max(owners, key=len)
        key = e[len(f"KBJ_{name}_"):]
        if key not in tables[name]:
            errs.append(f"{name}: the header's {e} has no key {key!r} in layout.{name}")
    return errs


# ---- the mirrors as they are ----
def test_structs(rep):
    for cname, cls in B.STRUCTS.items():
        assert not struct_errors(rep, cname, cls), "\n".join(struct_errors(rep, cname, cls))
    assert all(k != "?" for fs in rep.fields.values() for _, _, k in fs.values())            # no field of a type the kinds do not tell apart
    print(f"checked {len(B.STRUCTS)} structs, {sum(len(fs) for fs in rep.fields.values())} fields")


def test_tables(rep):
    tables = P.layout_tables()
    for name, table in tables.items():
        assert not table_errors(rep, name, table), "\n".join(table_errors(rep, name, table))
    assert list(L.REW.values()) == list(range(L.NREW)) and len(constants.REWARD_NAMES) == L.NREW
    for key, name in zip(L.REW, constants.REWARD_NAMES):                                      # KBJ_REW_* in constants.REWARD_NAMES order
        assert name.upper() in (key, key + "_P"), (key, name)
    print(f"checked {len(P.TABLE_NAMES)} tables and {len(P.FAMILY_NAMES)} families, {sum(len(t) for t in tables.values())} enumerators")


def test_constants(rep):
    for d in P.INT_DEFINES:
        assert rep.ints[f"KBJ_{d}"] == getattr(L, d), (d, rep.ints[f"KBJ_{d}"], getattr(L, d))
    for d in P.FLOAT_DEFINES:
        assert rep.floats[f"KBJ_{d}"] == getattr(L, d), (d, rep.floats[f"KBJ_{d}"], getattr(L, d))
    assert list(rep.ld_of) == list(P.LD_OF_RANGE)
    for n, ld in rep.ld_of.items():
        assert L.ld_of(n) == ld, (n, ld, L.ld_of(n))


def test_prototypes(rep):
    for name, sig in B.SIGNATURES.items():
        assert not signature_errors(rep, name, sig), "\n".join(signature_errors(rep, name, sig))
    assert all("?" not in p for p in rep.prototypes.values())
    print(f"checked {len(B.SIGNATURES)} prototypes")


def test_the_header_defines_nothing_without_a_mirror(text):
    assert header_structs(text) == set(B.STRUCTS), header_structs(text) ^ set(B.STRUCTS)
    assert header_functions(text) == set(B.SIGNATURES), header_functions(text) ^ set(B.SIGNATURES)
    assert len(header_enumerators(text)) > 300
    assert not enumerator_errors(text, P.layout_tables()), "\n".join(enumerator_errors(text, P.layout_tables()))
    assert set(P.TABLE_NAMES + list(P.FAMILY_NAMES)) == {k for k, v in vars(L).items() if k.isupper() and isinstance(v, dict)}     # and layout.py no table the probe is not asked for


def test_a_name_the_header_lacks_is_reported_with_the_compilers_message(tmp_path):
    with pytest.raises(P.ProbeError, match="KBJ_EP_NO_SUCH_COLUMN"):
        P.probe(str(tmp_path), structs={}, tables={"EP": {"NO_SUCH_COLUMN": 0}}, signatures={})


# ---- the checks reject mutated mirrors ----
def _restruct(cls, edit):
    fields = list(cls._fields_)
    edit(fields)
    return type(cls.__name__ + "Mutant", (C.Structure,), {"_fields_": fields})


def test_the_checks_reject_their_mutants(rep, text):
    names = [n for n, _ in L.Config._fields_]
    # (a) two adjacent float fields of kbj_config exchanged: same size, as the former check asked
    k = names.index("gamma")
    assert L.Config._fields_[k][1] is f32 and L.Config._fields_[k + 1] == ("lam", f32)

    def swap(fields):
        fields[k], fields[k + 1] = fields[k + 1], fields[k]
    mutant = _restruct(L.Config, swap)
    errs = struct_errors(rep, "kbj_config", mutant)
    assert C.sizeof(mutant) == C.sizeof(L.Config) == rep.sizeof["kbj_config"]
    assert len(errs) == 2 and errs[0].startswith("kbj_config.lam:") and errs[1].startswith("kbj_config.gamma:"), errs
    # (b) gae_terminal_value as a float: same size, same offsets
    k = names.index("gae_terminal_value")

    def retype(fields):
        fields[k] = ("gae_terminal_value", f32)
    mutant = _restruct(L.Config, retype)
    errs = struct_errors(rep, "kbj_config", mutant)
    assert C.sizeof(mutant) == C.sizeof(L.Config) and L.Config._fields_[k][1] is i32
    assert len(errs) == 1 and errs[0].startswith("kbj_config.gae_terminal_value:") and "'i'" in errs[0] and "'f'" in errs[0], errs
    # (c) one EP offset off by one
    errs = table_errors(rep, "EP", dict(L.EP, MASS=L.EP["MASS"] + 1))
    assert len(errs) == 1 and errs[0].startswith("EP: MASS is 72 in the header, 73"), errs
    # (d) a key removed from TRK: every remaining value is right, the header's enumerator has lost its mirror
    tables = P.layout_tables()
    tables["TRK"] = {k: v for k, v in L.TRK.items() if k != "SUMSQ"}
    assert not table_errors(rep, "TRK", tables["TRK"])
    errs = enumerator_errors(text, tables)
    assert len(errs) == 1 and errs[0].startswith("TRK: the header's KBJ_TRK_SUMSQ has no key"), errs
    # (e) an entry with its last argument dropped
    res, args = B.SIGNATURES["kbj_rollout"]
    errs = signature_errors(rep, "kbj_rollout", (res, args[:-1]))
    assert len(errs) == 1 and errs[0].startswith("kbj_rollout: takes 6 arguments") and "5 (" in errs[0], errs
    # (f) kbj_policy_step with step_index (uint32) and argmax (int) exchanged: the names are all there, as the former check asked
    res, args = B.SIGNATURES["kbj_policy_step"]
    assert (args[6], args[7]) == (C.c_uint32, C.c_int)
    mutated = dict(B.SIGNATURES, kbj_policy_step=(res, args[:6] + [args[7], args[6]] + args[8:]))
    assert set(mutated) == header_functions(text)
    errs = signature_errors(rep, "kbj_policy_step", mutated["kbj_policy_step"])
    assert errs == ["kbj_policy_step: argument 6 is u in the header, i in SIGNATURES", "kbj_policy_step: argument 7 is i in the header, u in SIGNATURES"], errs
    # (g) a header with one more enumerator in the AUX enum, without an initialiser
    grown, n = re.subn(r"(KBJ_AUX_SIZE\s*=\s*72)", r"\1,\n  KBJ_AUX_NEW_WORD", text)
    assert n == 1 and not enumerator_errors(text, P.layout_tables())
    errs = enumerator_errors(grown, P.layout_tables())
    assert len(errs) == 1 and errs[0].startswith("AUX: the header's KBJ_AUX_NEW_WORD has no key"), errs
