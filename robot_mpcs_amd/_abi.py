"""The ctypes view of ``include/rmpc.h``, read from the header itself: ``constants``, ``structs``, ``prototypes``.

Not a C parser.  After comments and preprocessor lines are taken out, the header may hold only
  * ``#define RMPC_X <integer>`` or ``(-<integer>)`` (other macros are not constants and are passed over),
  * ``typedef struct NAME { ... } NAME;`` whose members are ``[const] T [*]name[[extent]...]``, several declarators per
    declaration allowed, T one of int32_t, int64_t, double, int (void and char behind a pointer), an extent a literal
    or a constant; every pointer member is a ``c_void_p``,
  * ``typedef struct rmpc_handle rmpc_handle;`` and the ``extern "C"`` braces,
  * prototypes ``T [*]name(parameters);`` over any number of lines, with (long long too)
      ``const char *`` / ``char *`` -> ``c_char_p``; ``rmpc_handle *`` -> ``c_void_p``, ``**`` -> ``POINTER(c_void_p)``;
      a pointer to one of the structs -> ``POINTER(that Structure)``;
      ``void *`` and any pointer named ``d_*`` (a device pointer: the wrappers pass ``data_ptr()``) -> ``c_void_p``;
      every other ``T *p`` or ``T p[n]`` (a host array: the wrappers pass typed numpy pointers) -> ``POINTER(T)``.
Anything else -- unsigned, a union, a bit-field, a function pointer, an unknown type or extent, a stray declaration --
raises ``RmpcError`` with the text that was not understood; nothing is skipped.

The headers beside it are read the same way into tables of their own: ``include/rmpc_grid_large.h`` into
``large_constants`` / ``large_prototypes``, ``include/rmpc_assign_opt.h`` into ``assign_constants`` /
``assign_prototypes``, ``include/rmpc_tours.h`` into ``tours_constants`` / ``tours_prototypes``,
``include/rmpc_timed_tours.h`` into ``timed_tours_constants`` / ``timed_tours_structs`` / ``timed_tours_prototypes``,
``include/rmpc_timed_replan.h`` into ``timed_replan_constants`` / ``timed_replan_structs`` / ``timed_replan_prototypes``
(it takes a pointer to the timed tours' struct, which ``parse`` is told of; uint64_t, the word of its reservation table,
is typed for it), ``include/rmpc_timed_repair.h`` into ``timed_repair_constants`` / ``timed_repair_structs`` /
``timed_repair_prototypes``, ``include/rmpc_any_angle.h`` into ``any_angle_constants`` / ``any_angle_prototypes`` (its
work-size macro takes arguments: not a constant, passed over), ``include/rmpc_corridor.h`` into ``corridor_constants`` /
``corridor_prototypes`` (likewise), ``include/rmpc_traffic.h`` into ``traffic_constants`` / ``traffic_structs`` /
``traffic_prototypes``, ``include/rmpc_cbs.h`` into ``cbs_constants`` / ``cbs_structs`` / ``cbs_prototypes``,
``include/rmpc_ecbs.h`` into ``ecbs_constants`` / ``ecbs_structs`` / ``ecbs_prototypes``.
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmpc.h")
# the fields on large maps: a header of its own, read into tables of its own
LARGE_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_grid_large.h")
# the minimum-cost assignment: likewise
ASSIGN_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_assign_opt.h")
# the tours and the follower that stops: likewise
TOURS_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_tours.h")
# the timed tours: likewise, with a struct of its own
TIMED_TOURS_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_timed_tours.h")
# the lifelong timed tours: likewise
TIMED_REPLAN_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_timed_replan.h")
# the timed routes with repaired orders: likewise
TIMED_REPAIR_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_timed_repair.h")
# line of sight, shortened routes and the follower that looks ahead: likewise
ANY_ANGLE_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_any_angle.h")
# safe corridors from the map: likewise
CORRIDOR_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_corridor.h")
# traffic-aware routes: likewise, with a struct of its own
TRAFFIC_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_traffic.h")
# optimal timed routes: conflict-based search: likewise, with a struct of its own
CBS_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_cbs.h")
# bounded-suboptimal timed routes: focal conflict-based search: likewise
ECBS_HEADER = os.path.join(os.path.dirname(HEADER), "rmpc_ecbs.h")

_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int, "long long": C.c_longlong}
_DECLARATION = re.compile(r"(?:const\s+)?(long long|\w+)(\s+|\s*(?:\*\s*)+)(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)")


class RmpcError(RuntimeError):
    pass


def _extents(text, constants, where):
    out = []
    for e in re.findall(r"\w+", text):
        if not e.isdigit() and e not in constants:
            raise RmpcError(f"rmpc.h: unknown array extent {e!r} in {where!r}")
        out.append(int(e) if e.isdigit() else constants[e])
    return out


def _members(body, constants):
    """the ``_fields_`` of a struct body"""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (p.strip() for p in decl.split(","))
        m = _DECLARATION.fullmatch(first)
        if not m or m.group(1) not in (*_SCALARS, "void", "char"):
            raise RmpcError(f"rmpc.h: cannot type the member {decl!r}")
        base, parts = m.group(1), [m.groups()[1:]]
        for p in more:
            d = _DECLARATOR.fullmatch(p)
            if not d:
                raise RmpcError(f"rmpc.h: cannot type the member {decl!r}")
            parts.append(d.groups())
        for stars, name, ext in parts:
            if "*" not in stars and base not in _SCALARS:
                raise RmpcError(f"rmpc.h: cannot type the member {decl!r}")
            t = C.c_void_p if "*" in stars else _SCALARS[base]
            for n in reversed(_extents(ext, constants, decl)):      # double m[8][3] is (c_double * 3) * 8
                t = t * n
            fields.append((name, t))
    return fields


def _ctype(text, structs, constants, returns=False):
    """(name, ctypes type) of one parameter, or with ``returns`` a function's name and its return type"""
    m = _DECLARATION.fullmatch(text.strip())
    if not m:
        raise RmpcError(f"rmpc.h: cannot type {text.strip()!r}")
    base, name = m.group(1), m.group(3)
    depth = m.group(2).count("*") + len(_extents(m.group(4), constants, text))     # T p[n] is T *p
    if depth == 0 and base in _SCALARS:
        return name, _SCALARS[base]
    if depth == 1 and base == "char":
        return name, C.c_char_p
    if returns:
        if depth == 0 and base == "void":
            return name, None
    elif base == "rmpc_handle" and depth in (1, 2):
        return name, C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)
    elif depth == 1 and base in structs:
        return name, C.POINTER(structs[base])
    elif depth == 1 and (base == "void" or base in _SCALARS):
        return name, C.c_void_p if base == "void" or name.startswith("d_") else C.POINTER(_SCALARS[base])
    raise RmpcError(f"rmpc.h: cannot type {text.strip()!r}")


def parse(text, known=None):
    """(constants, structs, prototypes) of a header's text; ``known``: structs of a header it includes, which its
    prototypes may point to"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {k: int(a or b) for k, a, b in
                 re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RMPC_\w+)[ \t]+(?:(\d+)|\((-\d+)\))[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, braces = re.subn(r'\bextern\s+"C"\s*\{', "", text)
    structs = {}

    def take_struct(m):
        if m.group(1) != m.group(3):
            raise RmpcError(f"rmpc.h: struct {m.group(1)} is given the other name {m.group(3)}")
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": _members(m.group(2), constants)})
        return ""

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    prototypes = {}
    *statements, rest = text.split(";")
    for s in (s.strip() for s in statements):
        m = re.fullmatch(r"([^()]*)\((.*)\)", s, flags=re.S)
        if m:
            name, restype = _ctype(m.group(1), structs, constants, returns=True)
            args = [] if m.group(2).strip() == "void" else m.group(2).split(",")
            prototypes[name] = (restype, [_ctype(a, {**(known or {}), **structs}, constants)[1] for a in args])
        elif s.split() != "typedef struct rmpc_handle rmpc_handle".split():
            raise RmpcError(f"rmpc.h: not a form the binding knows: {s!r}")
    if rest.split() != ["}"] * braces:
        raise RmpcError(f"rmpc.h: not a form the binding knows: {rest.strip()!r}")
    return constants, structs, prototypes


def _read(path, known=None):
    try:
        with open(path) as f:
            return parse(f.read(), known)
    except OSError as e:
        raise RmpcError(f"{path} not found: the binding is derived from it ({e})") from None


constants, structs, prototypes = _read(HEADER)
large_constants, _, large_prototypes = _read(LARGE_HEADER)
assign_constants, _, assign_prototypes = _read(ASSIGN_HEADER)
tours_constants, _, tours_prototypes = _read(TOURS_HEADER)
timed_tours_constants, timed_tours_structs, timed_tours_prototypes = _read(TIMED_TOURS_HEADER)
timed_replan_constants, timed_replan_structs, timed_replan_prototypes = _read(TIMED_REPLAN_HEADER, timed_tours_structs)
timed_repair_constants, timed_repair_structs, timed_repair_prototypes = _read(TIMED_REPAIR_HEADER)
any_angle_constants, _, any_angle_prototypes = _read(ANY_ANGLE_HEADER)
corridor_constants, _, corridor_prototypes = _read(CORRIDOR_HEADER)
traffic_constants, traffic_structs, traffic_prototypes = _read(TRAFFIC_HEADER)
cbs_constants, cbs_structs, cbs_prototypes = _read(CBS_HEADER)
ecbs_constants, ecbs_structs, ecbs_prototypes = _read(ECBS_HEADER)
