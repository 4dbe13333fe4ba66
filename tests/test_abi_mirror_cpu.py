"""CPU (-m "not gpu"): radarslampy_amd/_abi.py against include/roam_abi.h, whole - every prototype (return type, argument count,
every scalar width, every typed pointee), every struct (field names, order, types, array lengths, offsets, size) and every constant
_abi mirrors.  A wrong width does not fail at the call, it hands the library a corrupted argument, so it has to fail here.  No
library is loaded and no device is used; the second test points the same comparison at tables that are wrong on purpose."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from radarslampy_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "roam_abi.h")

SCALARS = {"int32_t": (C.c_int32, np.int32, 4), "int64_t": (C.c_int64, np.int64, 8), "float": (C.c_float, np.float32, 4),
           "double": (C.c_double, np.float64, 8)}
RETURNS = {("int32_t", 0): C.c_int32, ("char", 1): C.c_char_p}
# header struct -> its mirror in _abi: a ctypes.Structure, or a numpy record dtype
STRUCTS = {"roam_engine_cfg": "EngineCfg", "roam_lane_result": "LaneResult", "roam_auto_prior_cfg": "AutoPriorCfg",
           "roam_pose_graph_opts": "PoseGraphOpts", "roam_icp_opts": "IcpOpts", "roam_keyframe_hdr": "KeyframeHdr",
           "roam_pose_graph_stats": "POSE_GRAPH_STATS", "roam_icp_stats": "ICP_STATS"}
# (header #define or enumerator, its name in _abi)
CONSTANTS = [(n, n) for n in ("ROAM_OK", "ROAM_E_ARG", "ROAM_E_HIP", "ROAM_E_CAPACITY", "ROAM_E_NODEVICE", "ROAM_E_STATE")] + [
    ("ROAM_" + n, n) for n in (
        "MAX_FEATURES", "WARP_POLAR_LOG", "WARP_POLAR_INVERSE", "WARP_AFFINE_INVERSE_MAP", "KLT_MAX_GUESS", "PRIOR_MAX_LINEAR",
        "FMT_MIN_R", "FMT_MAX_R", "STEP_NEW_SEQUENCE", "SCAN_CONTEXT_MAX_SECTORS", "SCAN_CONTEXT_MAX_RINGS", "SCAN_CONTEXT_MAX_CLIP",
        "LOOP_MAX_K", "LOOP_MAX_OFFSETS", "MAP_MAX_CELLS", "ICP_MAX_PAIRS", "ICP_MAX_POINTS", "ICP_MAX_COORD", "ICP_ITERATION_LIMIT",
        "ICP_OK", "ICP_MAX_ITERATIONS", "ICP_FEW_PAIRS", "TIME_FFT_FIVE", "TIME_DFT_FIVE", "TIME_FFT_ROWS", "TIME_FFT_TRANSPOSE",
        "TIME_FFT_COLS", "COMM_ID_BYTES")]


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def _decl(text):
    """'const roam_icp_opts *opts' -> ('roam_icp_opts', 1, 'opts'): the base type, the pointer depth, the name ('' without one)"""
    words = [w for w in re.findall(r"\w+", text) if w != "const"]
    return words[0], text.count("*"), words[1] if len(words) > 1 else ""


def parse_prototypes(text):
    """-> {entry: ((return base, pointer depth), [(base, pointer depth, name) per parameter])}"""
    out = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(roam_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() in ("", "void") else [_decl(p) for p in params.split(",")]
        assert name not in out, f"{name} declared twice"
        out[name] = (_decl(ret)[:2], params)
    return out


def parse_structs(text):
    """-> {struct: [(field, scalar type, array length or None)]}; 'int32_t a, b, c;' declares three fields"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(roam_\w+)\s*\{([^{}]*)\}\s*\1\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = decl.split(None, 1)
            for item in names.split(","):
                m = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", item)
                assert m, f"{name}: cannot read the declaration {decl!r}"
                fields.append((m[1], base, int(m[2]) if m[2] else None))
        out[name] = fields
    return out


def literal(text):
    """the value of a numeric C literal: decimal, hex, float with an exponent and / or an f suffix, a << b, parentheses"""
    t = text.strip()
    while t.startswith("(") and t.endswith(")"):
        t = t[1:-1].strip()
    shift = re.fullmatch(r"(\w+)\s*<<\s*(\w+)", t)
    if shift:
        return literal(shift[1]) << literal(shift[2])
    if re.fullmatch(r"[-+]?0[xX][0-9a-fA-F]+", t):
        return int(t, 16)
    if re.fullmatch(r"[-+]?\d+", t):
        return int(t)
    if re.fullmatch(r"[-+]?(\d+\.\d*|\.\d+|\d+)([eE][-+]?\d+)?[fF]?", t):
        return float(t.rstrip("fF"))
    raise ValueError(f"not a numeric literal: {text!r}")


def parse_constants(text):
    """-> {name: value} of every '#define ROAM_X literal' and every enumerator 'ROAM_X = literal'"""
    out = {m[1]: literal(m[2]) for m in re.finditer(r"(?m)^[ \t]*#[ \t]*define[ \t]+(ROAM_\w+)[ \t]+(\S.*?)[ \t]*$", text)}
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", text):
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, value = item.split("=")
            out[name.strip()] = literal(value)
    return out


def _ctype_name(t):
    return getattr(t, "__name__", repr(t))


def _pointer_types(base, depth, abi):
    """the ctypes a pointer parameter of the header may be bound as"""
    ok = [C.c_void_p]
    if depth == 2:
        ok.append(C.POINTER(C.c_char_p if base == "char" else C.c_void_p))      # a T ** handle: the address of a void pointer
    elif base == "char":
        ok.append(C.c_char_p)
    elif base in SCALARS:
        ok.append(C.POINTER(SCALARS[base][0]))
    elif base in STRUCTS and isinstance(getattr(abi, STRUCTS[base], None), type):
        ok.append(C.POINTER(getattr(abi, STRUCTS[base])))
    return ok


def _natural_layout(fields):
    """C's layout of scalar fields and arrays of them: every field aligned to its scalar's size -> ([offset per field], size)"""
    offsets, end, align = [], 0, 1
    for _, base, length in fields:
        size = SCALARS[base][2]
        end = -(-end // size) * size
        offsets.append(end)
        end += size * (length or 1)
        align = max(align, size)
    return offsets, -(-end // align) * align


def _mirror_fields(mirror):
    """a Structure or a record dtype -> ([(field, ctypes scalar, array length or None, offset)], size)"""
    if isinstance(mirror, np.dtype):
        back = {np.dtype(s[1]): s[0] for s in SCALARS.values()}
        out = []
        for name in mirror.names:
            dt, off = mirror.fields[name][:2]
            length = None if dt.subdtype is None else int(np.prod(dt.subdtype[1]))
            out.append((name, back.get(dt.base, dt.base), length, off))
        return out, mirror.itemsize
    out = []
    for name, t in mirror._fields_:
        length = getattr(t, "_length_", None)
        out.append((name, t._type_ if length else t, length, getattr(mirror, name).offset))
    return out, C.sizeof(mirror)


def mirror_mismatches(text, abi):
    """every disagreement between the header (comments stripped) and the mirror `abi` (radarslampy_amd._abi, or an object with its
    attributes), one string each; an empty list: the mirror is the header"""
    bad = []
    protos = parse_prototypes(text)
    for name in sorted(set(protos) ^ set(abi._SIGS)):
        bad.append(f"{name}: declared in {'the header' if name in protos else '_SIGS'} only")
    for name in sorted(set(protos) & set(abi._SIGS)):
        (ret, params), (res, args) = protos[name], abi._SIGS[name]
        if RETURNS.get(ret) is not res:
            bad.append(f"{name}: returns {_ctype_name(res)}, the header {ret[0]}{' *' * ret[1]}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(args)} arguments, the header {len(params)}")
            continue
        for i, ((base, depth, pname), got) in enumerate(zip(params, args)):
            said = f"{base}{' ' + '*' * depth if depth else ''} {pname}"
            if depth == 0:
                if base not in SCALARS:
                    bad.append(f"{name}: argument {i} ({said}): a scalar type this test does not know")
                elif got is not SCALARS[base][0]:
                    bad.append(f"{name}: argument {i} is {_ctype_name(got)}, the header {said}")
            elif not any(got is t for t in _pointer_types(base, depth, abi)):
                bad.append(f"{name}: argument {i} is {_ctype_name(got)}, the header {said}")
    structs = parse_structs(text)
    for sname in sorted(set(structs) ^ set(STRUCTS)):
        bad.append(f"{sname}: a struct of {'the header without a mirror' if sname in structs else 'this test that the header lacks'}")
    for sname in sorted(set(structs) & set(STRUCTS)):
        fields, mname = structs[sname], STRUCTS[sname]
        unknown = [f for f in fields if f[1] not in SCALARS]
        if unknown:
            bad.append(f"{sname}: field {unknown[0][0]} of type {unknown[0][1]}, which this test does not know")
            continue
        got, size = _mirror_fields(getattr(abi, mname))
        offsets, want_size = _natural_layout(fields)
        if [g[0] for g in got] != [f[0] for f in fields]:
            bad.append(f"{sname} / {mname}: fields {[g[0] for g in got]}, the header {[f[0] for f in fields]}")
            continue
        for (fname, base, length), off, (_, gtype, glength, goff) in zip(fields, offsets, got):
            if gtype is not SCALARS[base][0] or glength != length:
                bad.append(f"{sname} / {mname}: {fname} is {_ctype_name(gtype)}{'[%d]' % glength if glength else ''}, the header "
                           f"{base}{'[%d]' % length if length else ''}")
            elif goff != off:
                bad.append(f"{sname} / {mname}: {fname} at offset {goff}, natural alignment puts it at {off}")
        if size != want_size:
            bad.append(f"{sname} / {mname}: {size} bytes, natural alignment gives {want_size}")
    consts = parse_constants(text)
    for hname, aname in CONSTANTS:
        if hname not in consts:
            bad.append(f"{hname}: not a constant of the header")
        elif getattr(abi, aname) != consts[hname]:
            bad.append(f"{aname} = {getattr(abi, aname)!r}, the header's {hname} = {consts[hname]!r}")
    listed = {h for h, _ in CONSTANTS}
    for hname in sorted(set(consts) - listed):
        if hasattr(abi, hname) or hasattr(abi, hname[len("ROAM_"):]):
            bad.append(f"{hname}: mirrored by _abi but not in this test's table")
    return bad


def test_the_mirror_is_the_header():
    text = _header_text()
    protos, structs, consts = parse_prototypes(text), parse_structs(text), parse_constants(text)
    assert len(protos) >= 135 and len(structs) == 8 and len(consts) >= 30      # the parsers see the header
    assert set(protos) == set(_abi._SIGS) == set(_abi.ABI_SYMBOLS)
    assert consts["ROAM_MAP_MAX_CELLS"] == 1 << 26 and consts["ROAM_STEP_NEW_SEQUENCE"] == 0x40000000
    assert consts["ROAM_ICP_MAX_COORD"] == 1e6 and consts["ROAM_KLT_MAX_GUESS"] == 2.0 ** 20 and consts["ROAM_E_STATE"] == -5
    assert not set(_abi._SIGS) & set(_abi._INTERNAL_SIGS)
    assert mirror_mismatches(text, _abi) == []


def _with(**changed):
    return types.SimpleNamespace(**dict(vars(_abi), **changed))


def _sigs(name, edit):
    res, args = _abi._SIGS[name]
    return _with(_SIGS=dict(_abi._SIGS, **{name: (res, edit(list(args)))}))


def _fields(struct, edit):
    return type(struct.__name__, (C.Structure,), {"_fields_": edit(list(struct._fields_))})


def _swap(items, i, j):
    items[i], items[j] = items[j], items[i]
    return items


WRONG = {
    "pointee int64 -> int32": (lambda: _sigs("roam_loop_db_map_bounds", lambda a: a[:-1] + [C.POINTER(C.c_int32)]),
                               "roam_loop_db_map_bounds: argument 5 is "),
    "an argument dropped": (lambda: _sigs("roam_warp_affine_f32", lambda a: a[:-1]), "roam_warp_affine_f32: 12 arguments, the header 13"),
    "double as float": (lambda: _sigs("roam_warp_polar_f32", lambda a: a[:12] + [C.c_float] + a[13:]),
                        "roam_warp_polar_f32: argument 12 is c_float, the header double max_radius"),
    "struct field narrowed": (lambda: _with(EngineCfg=_fields(_abi.EngineCfg, lambda f: [(n, C.c_int32 if n == "clique_node_limit" else t)
                                                                                         for n, t in f])),
                              "roam_engine_cfg / EngineCfg: clique_node_limit is "),
    "struct fields exchanged": (lambda: _with(IcpOpts=_fields(_abi.IcpOpts, lambda f: _swap(f, 2, 3))),
                                "roam_icp_opts / IcpOpts: fields ['gate_start', 'gate_end', 'max_iterations', 'gate_decay'"),
    "constant off by one": (lambda: _with(LOOP_MAX_K=_abi.LOOP_MAX_K + 1), "LOOP_MAX_K = 33, the header's ROAM_LOOP_MAX_K = 32"),
}


@pytest.mark.parametrize("case", list(WRONG))
def test_a_wrong_mirror_is_reported(case):
    make, said = WRONG[case]
    assert _abi._SIGS["roam_loop_db_map_bounds"][1][-1] is C.POINTER(C.c_int64)        # a typed pointer, so its pointee can be wrong
    bad = mirror_mismatches(_header_text(), make())
    assert any(b.startswith(said) for b in bad), bad
