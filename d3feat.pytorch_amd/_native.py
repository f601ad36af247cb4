"""ctypes binding of ``libd3feat_hip.so`` (the C ABI declared in ``include/d3feat_hip.h``).

There is deliberately NO fallback: if the HIP library is missing or a tensor is not a CUDA/HIP tensor, every
operator raises ``RuntimeError`` (the reference's only error type, cpp_neighbors/wrapper.cpp:77).
"""
import ctypes as C
import os
import re
import subprocess

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_PKG_DIR)
LIB_PATH = os.path.join(_PKG_DIR, "libd3feat_hip.so")
CSRC = os.path.join(_PKG_DIR, "csrc")
SOURCES = ["radius_neighbors.hip", "grid_subsample.hip", "kpconv.hip", "kpconv_fused.hip", "kpconv_aggregate.hip", "kpconv_small.hip", "kpconv_deform.hip", "pool.hip", "detection.hip", "loss.hip",
           "reverse_table.hip", "kpconv_dx_gather.hip", "matching.hip", "elementwise.hip", "batchnorm.hip", "linear.hip", "gemm_epilogue.hip", "optimizer.hip", "misc.hip",
           "registration.hip", "nearest_pairs.hip", "icp.hip", "normals.hip", "augment.hip", "posegraph.hip", "tsdf.hip", "tsdf_integrate.hip", "tsdf_extract.hip", "tsdf_mesh.hip", "tsdf_sparse.hip", "odometry.hip", "tsdf_raycast.hip",
           "tsdf_mesh_sparse.hip", "fpfh.hip", "fgr.hip", "iss.hip", "sc2.hip", "knn_match.hip"]

# The binding is READ from the header, once, at import: prototypes, struct layouts and integer #defines are stated there
# alone.  What the closed type map below cannot take raises; nothing in the header is skipped.
HEADER = os.path.join(_REPO, "include", "d3feat_hip.h")
_SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
            "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_POINTEES = set(_SCALARS) | {"char", "uint8_t"}     # what a c_void_p may point to, besides the structs
_STRUCT = r"typedef\s+struct\s+(%s)\s*\{(.*?)\}\s*\1\s*;"


def _code(text):
    """The header without its comments and its extern "C" guards."""
    return re.sub(r"#ifdef __cplusplus\n.*?#endif", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S)


def _declaration(text, structs, where):
    """'const float* x' -> ('x', c_void_p), 'double R[9]' -> ('R', c_double * 9), 'int' -> ('', c_int)."""
    m = re.fullmatch(r"\s*(\w+)\s*((?:\*\s*)*)(\w*)\s*(?:\[(\d+)\])?\s*", re.sub(r"\bconst\b", " ", text))
    base, stars = (m.group(1), m.group(2).count("*")) if m else (None, 0)
    if stars == 0 and base in _SCALARS:
        ctype = _SCALARS[base]
    elif stars == 1 and base == "char":
        ctype = C.c_char_p
    elif stars == 1 and base in structs:
        ctype = C.POINTER(structs[base])
    elif stars and (base in _POINTEES or base in structs):
        ctype = C.c_void_p
    else:
        raise RuntimeError("d3feat_hip.h: %s: no ctypes type for %r" % (where, " ".join(text.split())))
    return m.group(3), ctype * int(m.group(4)) if m.group(4) else ctype


def parse_struct(text, name):
    """The _fields_ of `typedef struct name { ... } name;`, one per declarator ('int32_t N, Cin;' holds two)."""
    m = re.search(_STRUCT % name, _code(text), flags=re.S)
    if not m:
        raise RuntimeError("d3feat_hip.h: no struct %s" % name)
    fields = []
    for line in filter(str.strip, m.group(2).split(";")):
        first, *others = re.sub(r"\bconst\b", " ", line).split(",")
        base = re.match(r"\s*\w*", first).group(0)
        fields += [_declaration(d, {}, "struct " + name) for d in [first] + [base + " " + d for d in others]]
    if not all(field for field, _ in fields):
        raise RuntimeError("d3feat_hip.h: struct %s: a field without a name" % name)
    return fields


def parse_defines(text):
    """{D3F_X: value} of every #define D3F_X <integer expression>; the expression may name earlier defines."""
    out = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(D3F_\w+)(.*)$", _code(text), flags=re.M):
        try:
            plain = re.sub(r"\bD3F_\w+", lambda m: "(%d)" % out[m.group(0)], expr)
            value = eval(plain, {"__builtins__": {}}) if re.fullmatch(r"[\s0-9a-fA-FxX()+\-*<>|&~^]+", plain) else None
        except Exception:       # a define that is not (yet) there, a syntax error
            value = None
        if type(value) is int:
            out[name] = value
        elif name != "D3F_SPACK_READY":         # a pointer cast, the one define that is no integer: ops.SPACK_READY
            raise RuntimeError("d3feat_hip.h: #define %s %s: no integer expression" % (name, expr.strip()))
    return out


def parse_prototypes(text, structs):
    """{name: (restype, [argtypes])}.  Every statement outside the structs has to be one prototype of a d3f_ function,
    and every `d3f_<name>(` in the header one of them."""
    code = re.sub(_STRUCT % r"\w+", "", re.sub(r"^[ \t]*#.*$", "", _code(text), flags=re.M), flags=re.S)
    out = {}
    for st in filter(str.strip, re.split(r"(?<=;)", code)):        # each statement with its ';'
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(d3f_\w+)\s*\(([^()]*)\)\s*;", st)
        if not m or m.group(2) in out:
            raise RuntimeError("d3feat_hip.h: not one whole, new prototype: %r" % " ".join(st.split())[:200])
        name, params = m.group(2), [] if m.group(3).strip() == "void" else m.group(3).split(",")
        out[name] = (_declaration(m.group(1), structs, name + ", return type")[1],
                     [_declaration(p, structs, name)[1] for p in params])
    if len(re.findall(r"\bd3f_\w+\s*\(", _code(text))) != len(out):
        raise RuntimeError("d3feat_hip.h: d3f_<name>( occurs outside the %d prototypes" % len(out))
    return out


with open(HEADER) as _f:
    _TEXT = _f.read()


class Tunables(C.Structure):
    """d3f_tunables of include/d3feat_hip.h: the library's knobs (it never reads the environment)."""
    _fields_ = parse_struct(_TEXT, "d3f_tunables")


class AtbProblem(C.Structure):
    """d3f_atb_problem of include/d3feat_hip.h: one queued weight gradient grad_w [Cout, ldw] = grad_out^T x."""
    _fields_ = parse_struct(_TEXT, "d3f_atb_problem")


class AugmentJob(C.Structure):
    """d3f_augment_job of include/d3feat_hip.h: one training item of the resident 3DMatch split."""
    _fields_ = parse_struct(_TEXT, "d3f_augment_job")


STRUCTS = {"d3f_tunables": Tunables, "d3f_atb_problem": AtbProblem, "d3f_augment_job": AugmentJob}
SIGNATURES = parse_prototypes(_TEXT, STRUCTS)   # name -> (restype, argtypes)
DEFINES = parse_defines(_TEXT)                  # every integer #define D3F_X; each also a module attribute _native.D3F_X
globals().update(DEFINES)
del _f, _TEXT

ERRORS = {DEFINES["D3F_" + name]: text for name, text in (
    ("EINVAL", "invalid argument"), ("EWORKSPACE", "workspace too small"), ("ELAUNCH", "HIP launch failure"))}
STATUS_BITS = {DEFINES["D3F_ST_" + name]: text for name, text in (
    ("CAND_OVERFLOW", "a query has more in-radius candidates than the kernel can rank (512; fpfh: 2^18 neighbours of a point)"),
    ("CELL_RANGE", "a point lies outside the addressable cell grid"),
    ("TABLE_FULL", "voxel hash table full"),
    ("CAPACITY", "a pyramid level needs more rows than its capacity (raise the capacities)"),
    ("WIDE_OVERFLOW", "a point has more in-radius neighbors than the reverse (wide) table holds"),
    ("NO_NEAREST", "an upsampling query has no coarse point within the guaranteed nearest bound (a coarse level lost voxels, "
                   "or the bound passed to query_prefix is wrong)"))}


def build(verbose=False, jobs=None, extra_flags=(), out=None, objdir=None):
    """Compile every HIP source for gfx950 into the in-tree shared library (cross-compiles without a GPU).
    One object per source under ``build/`` (recompiled only when the source or a header changed), then one link.
    ``extra_flags`` / ``out`` / ``objdir``: a MEASUREMENT build of the same sources next to the product (e.g.
    -DD3F_ATB_PROBE=1 into profiles/experiments/, profiles/atb_loop_probe.py); the product build takes neither."""
    # -ffp-contract=off: HIP's __fmul_rn/__fadd_rn are plain operators on AMD, so with the default contract=fast
    # the compiler fuses the "exact" d2 = (dx*dx + dy*dy) + dz*dz into FMAs and the strict d2 < r2 test / the
    # distance order stop matching the reference's x86 arithmetic bit for bit.  Fusion is requested explicitly
    # (fmaf / MFMA) where it is wanted.
    from concurrent.futures import ThreadPoolExecutor
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC",
             "-I" + os.path.join(_REPO, "include")] + list(extra_flags)
    objdir = objdir or os.path.join(_PKG_DIR, "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    headers.append(os.path.join(_REPO, "include", "d3feat_hip.h"))
    hdr_time = max(os.path.getmtime(h) for h in headers)

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        path = os.path.join(CSRC, src)
        if os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(path), hdr_time):
            return obj
        cmd = ["hipcc"] + flags + ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out or LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out or LIB_PATH


def _needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_REPO, "include", "d3feat_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


_lib = None


def lib():
    """The loaded library; raises RuntimeError if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        try:  # bring up torch's HIP context first: the library shares torch's bundled HIP runtime
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:  # pragma: no cover
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libd3feat_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  d3feat_pytorch_amd has no CPU or PyTorch fallback.")
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


TRACE = False     # debugging: name every C-ABI call on stderr and fence it (set _native.TRACE = True)


def check(rc, what):
    if TRACE:  # debugging aid: name every C-ABI call and fence it, so a device fault can be attributed
        import sys
        import torch
        sys.stderr.write("[d3f] %s\n" % what)
        sys.stderr.flush()
        torch.cuda.synchronize()
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, ERRORS.get(rc, "error %d" % rc)))


def set_tunables(**kw):
    """Change fields of the library's d3f_tunables (experiments / tests); returns the previous values as a dict."""
    L = lib()
    t = Tunables()
    L.d3f_get_tunables(C.byref(t))
    old = {name: getattr(t, name) for name, _ in Tunables._fields_ if name != "reserved"}
    for k, v in kw.items():
        if k not in old:
            raise RuntimeError("d3f_tunables has no field %r" % k)
        setattr(t, k, int(v))
    check(L.d3f_set_tunables(C.byref(t)), "d3f_set_tunables")
    return old


def status_message(word):
    return "; ".join(msg for bit, msg in STATUS_BITS.items() if word & bit)
