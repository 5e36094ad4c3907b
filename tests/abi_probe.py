"""What the host C++ compiler says of include/kbj.h, asked for exactly the names the Python mirrors use (spec/layout.py, host/binding.py).

probe() writes one C++17 source from the mirrors - a line of printf per struct, field, enumerator, constant and prototype -, compiles it
with g++ against the header, runs it and returns the parsed lines. The header is parsed by the compiler, not by a regex: enumerators
written as expressions or left implicit, nested arrays, padding and typedef'd integer types come out as what they are. Nothing of the
library is linked (prototypes are read through decltype, which needs no definition), so this needs neither hipcc nor a GPU.
tests/test_abi_mirror.py compares the result with ctypes; other host tests may read it too (report() compiles once per process)."""
import contextlib
import ctypes as C
import os
import subprocess
import tempfile
from dataclasses import dataclass, field

from kbot_joystick_amd.host import binding as B
from kbot_joystick_amd.spec import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# the record-offset tables of layout.py: KBJ_<name>_<key> for every key (OBS holds (offset, width) pairs: the offset is the enumerator)
TABLE_NAMES = ("OBS EP ES RC AUX QSTATE EACC EPST CMODE TERR TACC TRK GACC GAIT GFOOT GENV AACC ACT AJNT AENV POUT PREC PSTAT "
               "SSIG SOUT SREC SSTAT FOUT FREC FSTAT PERT RREC RSTAT").split()
# enumerators that are no record offsets, mirrored all the same: the reward slots and the threefry stream ids
FAMILY_NAMES = ("REW", "RNG")


def layout_tables(names=TABLE_NAMES + list(FAMILY_NAMES)):
    """name -> {key: value} of the named layout tables."""
    return {n: {k: (v[0] if isinstance(v, tuple) else v) for k, v in getattr(L, n).items()} for n in names}


# numeric #defines that layout.py restates: KBJ_<name>, integers and floats
INT_DEFINES = ("NBODY NQ NV NU NCAP NCON NCMD NREW NOBS_ACTOR NOBS_CRITIC LD_ACTOR LD_CRITIC MAX_EXTRA_OBS MAGIC VERSION NTERR NPEAK NSCH "
               "FREC_NSUMS").split()
FLOAT_DEFINES = ("PUSH_NEVER", "OBS_JVEL_DIV", "OBS_ACTFRC_DIV")
LD_OF_RANGE = range(0, 601)      # KBJ_LD_OF(n) against layout.ld_of: every width a context can have (475 + 64 user columns) and beyond

# kind letters. Fields: f float, d double, i int32, u uint32, p pointer, c char. Arguments and results: those, z size_t, l int64.
_KINDS = {C.c_float: "f", C.c_double: "d", C.c_int32: "i", C.c_uint32: "u", C.c_void_p: "p", C.c_char_p: "p", C.c_char: "c",
          C.c_size_t: "z", C.c_int64: "l"}


def ctypes_kind(t) -> str:
    """The kind letter of a ctypes type: arrays by their element type, every pointer 'p', '?' for a type the ABI does not use."""
    while isinstance(t, type) and issubclass(t, C.Array):
        t = t._type_
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "p"
    return _KINDS.get(t, "?")


def ctypes_fields(cls):
    """[(name, offset, size, kind)] of a ctypes.Structure, in declaration order."""
    return [(n, getattr(cls, n).offset, getattr(cls, n).size, ctypes_kind(t)) for n, t in cls._fields_]


def ctypes_signature(sig) -> str:
    """'r:aaa' of a SIGNATURES entry (restype, argtypes): the result's kind, then one letter per argument."""
    return ctypes_kind(sig[0]) + ":" + "".join(ctypes_kind(a) for a in sig[1])


class ProbeError(RuntimeError):
    """The probe did not compile or run: the message is the compiler's (a name of the mirrors that the header lacks shows up here)."""


@dataclass
class Report:
    sizeof: dict = field(default_factory=dict)        # C struct name -> bytes
    fields: dict = field(default_factory=dict)        # C struct name -> {field: (offset, size, kind)}
    enums: dict = field(default_factory=dict)         # KBJ_X_Y -> value
    ints: dict = field(default_factory=dict)          # KBJ_X -> value
    floats: dict = field(default_factory=dict)        # KBJ_X -> value, exact
    ld_of: dict = field(default_factory=dict)         # n -> KBJ_LD_OF(n)
    prototypes: dict = field(default_factory=dict)    # kbj_name -> 'r:aaa'


_PRELUDE = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "kbj.h"

template <class T> constexpr char kind() {
  using U = std::remove_cv_t<T>;
  if constexpr (std::is_pointer_v<U>) return 'p';
  else if constexpr (std::is_same_v<U, float>) return 'f';
  else if constexpr (std::is_same_v<U, double>) return 'd';
  else if constexpr (std::is_same_v<U, int32_t>) return 'i';
  else if constexpr (std::is_same_v<U, uint32_t>) return 'u';
  else if constexpr (std::is_same_v<U, char>) return 'c';
  else if constexpr (std::is_same_v<U, size_t>) return 'z';
  else if constexpr (std::is_same_v<U, int64_t>) return 'l';
  else return '?';
}
template <class F> struct proto;
template <class R, class... A> struct proto<R (*)(A...)> {
  static void print(const char* name) {
    std::printf("P %s %c:", name, kind<R>());
    (std::putchar(kind<A>()), ...);
    std::putchar('\n');
  }
};
#define STRUCT(T) std::printf("S %s %zu\n", #T, sizeof(T))
#define FIELD(T, f) std::printf("F %s %s %zu %zu %c\n", #T, #f, offsetof(T, f), sizeof(T::f), kind<std::remove_all_extents_t<decltype(T::f)>>())
#define ENUM(e) std::printf("E %s %lld\n", #e, (long long)(e))
#define INT(d) std::printf("I %s %lld\n", #d, (long long)(d))
#define FLOAT(d) std::printf("X %s %a\n", #d, (double)(d))
#define PROTO(f) proto<decltype(&f)>::print(#f)

int main() {
"""


def source(structs, tables, signatures, int_defines=(), float_defines=(), ld_of=()) -> str:
    """The probe's C++ text for these mirrors (structs: C name -> ctypes class, tables: name -> {key: value}, signatures: name -> entry)."""
    out = [_PRELUDE]
    for cname, cls in structs.items():
        out.append(f"  STRUCT({cname});")
        out += [f"  FIELD({cname}, {n});" for n, _ in cls._fields_]
    out += [f"  ENUM(KBJ_{t}_{k});" for t, table in tables.items() for k in table]
    out += [f"  INT(KBJ_{d});" for d in int_defines]
    out += [f"  FLOAT(KBJ_{d});" for d in float_defines]
    if len(ld_of):
        out.append(f"  for (int n = {ld_of[0]}; n <= {ld_of[-1]}; ++n) std::printf(\"L %d %d\\n\", n, KBJ_LD_OF(n));")
    out += [f"  PROTO({name});" for name in signatures]
    out.append("  return 0;\n}\n")
    return "\n".join(out)


def probe(build_dir, **mirrors) -> Report:
    """Compile source(**mirrors) in build_dir, run it and parse what it prints. ProbeError carries the compiler's message."""
    src, exe = os.path.join(build_dir, "abi_probe.cpp"), os.path.join(build_dir, "abi_probe")
    with open(src, "w") as f:
        f.write(source(**mirrors))
    cc = subprocess.run(["g++", "-std=c++17", "-O0", "-I" + INCLUDE, "-o", exe, src], capture_output=True, text=True)
    if cc.returncode != 0:
        raise ProbeError("the ABI probe does not compile against include/kbj.h:\n" + cc.stderr)
    run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0:
        raise ProbeError(f"the ABI probe exited with {run.returncode}:\n{run.stderr}")
    r = Report()
    for line in run.stdout.splitlines():
        tag, *w = line.split()
        if tag == "S":
            r.sizeof[w[0]] = int(w[1])
            r.fields[w[0]] = {}
        elif tag == "F":
            r.fields[w[0]][w[1]] = (int(w[2]), int(w[3]), w[4])
        elif tag == "E":
            r.enums[w[0]] = int(w[1])
        elif tag == "I":
            r.ints[w[0]] = int(w[1])
        elif tag == "X":
            r.floats[w[0]] = float.fromhex(w[1])
        elif tag == "L":
            r.ld_of[int(w[0])] = int(w[1])
        elif tag == "P":
            r.prototypes[w[0]] = w[1]
        else:
            raise ProbeError(f"unexpected line from the ABI probe: {line!r}")
    return r


_report = None


def report(build_dir=None) -> Report:
    """The probe of the package's own mirrors, compiled once per process (in build_dir, e.g. a pytest tmp dir; without one in a
    temporary directory of its own)."""
    global _report
    if _report is None:
        with tempfile.TemporaryDirectory(prefix="kbj_abi_probe_") if build_dir is None else contextlib.nullcontext(str(build_dir)) as d:
            _report = probe(d, structs=B.STRUCTS, tables=layout_tables(), signatures=B.SIGNATURES, int_defines=INT_DEFINES,
                            float_defines=FLOAT_DEFINES, ld_of=LD_OF_RANGE)
    return _report
