"""CPU: the C-ABI library loads and exports every symbol include/d3feat_hip.h declares; the ctypes binding is read
from that header (prototypes, structs, integer defines), strictly, and agrees with what the C compiler makes of it."""
import ast
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import d3feat_pytorch_amd
from d3feat_pytorch_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(REPO, "include", "d3feat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(d3f_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "libd3feat_hip.so does not export %s" % n


def test_ctypes_table_covers_header():
    assert sorted(_native.SIGNATURES) == _declared()


def test_the_generated_surface_prototypes_are_the_sixteen_literal_ones():
    """The extract and mesh prototypes as they were once written out by hand, entry by entry, against what the header
    yields."""
    C = ctypes
    _vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    literal = {
        "d3f_tsdf_extract_ws_bytes": (_sz, [C.c_int64]),
        "d3f_tsdf_extract_count": (_i, [_vp, _vp, _vp, _vp, _i, C.c_int64, _f, _vp, _vp, _sz, _vp]),
        "d3f_tsdf_extract": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, _f, _i, C.c_int64, _vp, _vp, _vp, _vp, _sz,
                                  _vp]),
        "d3f_tsdf_extract_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, _f, C.c_int64, _vp, _vp, _vp]),
        "d3f_tsdf_sparse_extract_ws_bytes": (_sz, [C.c_int64]),
        "d3f_tsdf_sparse_extract_count": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f, _vp, _vp,
                                               _sz, _vp]),
        "d3f_tsdf_sparse_extract": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f, _i,
                                         C.c_int64, _vp, _vp, _vp, _vp, _sz, _vp]),
        "d3f_tsdf_sparse_extract_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f,
                                              C.c_int64, _vp, _vp, _vp]),
        "d3f_tsdf_mesh_ws_bytes": (_sz, [C.c_int64]),
        "d3f_tsdf_mesh_count": (_i, [_vp, _vp, _vp, _vp, _i, C.c_int64, _f, _vp, _vp, _vp, _sz, _vp]),
        "d3f_tsdf_mesh": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, _f, _i, C.c_int64, C.c_int64, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _sz, _vp]),
        "d3f_tsdf_mesh_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, _f, C.c_int64, C.c_int64, _vp, _vp, _vp,
                                    _vp, _vp, _vp]),
        "d3f_tsdf_sparse_mesh_ws_bytes": (_sz, [C.c_int64]),
        "d3f_tsdf_sparse_mesh_count": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f, _vp, _vp, _vp,
                                            _sz, _vp]),
        "d3f_tsdf_sparse_mesh": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f, _i,
                                      C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
        "d3f_tsdf_sparse_mesh_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_int64, C.c_int64, _f,
                                           C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    }
    for name, prototype in literal.items():
        assert _native.SIGNATURES[name] == prototype, name
    assert "tsdf_extract.hip" in _native.SOURCES


def test_prototypes_of_every_other_type_class_are_the_literal_ones():
    """char* both ways, a void return, pointers to the three structs, int64_t / uint64_t / uint32_t / double by value and
    as return types, void* const*: the hand-written entries of these twelve, as they stood before the table was derived."""
    C = ctypes
    _vp, _i, _f, _sz, _d = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_double
    literal = {
        "d3f_version": (C.c_char_p, []),
        "d3f_device_arch_name": (_i, [C.c_char_p, _i]),
        "d3f_debug_set_flags": (None, [_i]),
        "d3f_get_tunables": (None, [C.POINTER(_native.Tunables)]),
        "d3f_linear_grad_weight_group": (_i, [C.POINTER(_native.AtbProblem), _i, _vp, _sz, _vp]),
        "d3f_augment_pairs": (_i, [_vp, C.c_int64, _vp, C.c_int64, C.POINTER(_native.AugmentJob), _i, _i, _d, _vp, _sz, _vp]),
        "d3f_augment_key_host": (C.c_uint64, [C.c_uint64, _i, C.c_uint32]),
        "d3f_ransac_rigid": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, _i, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _sz, _vp]),
        "d3f_copy_buffers": (_i, [_vp, _vp, _vp, _vp, _i, C.c_double, _vp]),
        "d3f_zero_buffers": (_i, [_vp, _vp, _i, _vp]),
        "d3f_depth_pyramid_pixels": (C.c_int64, [_i, _i, _i]),
        "d3f_icp_rigid_color": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _i, C.c_int64, _vp, _d, _i, _d, _d,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    }
    for name, prototype in literal.items():
        assert _native.SIGNATURES[name] == prototype, name


@pytest.mark.parametrize("text, names", [
    ("int d3f_f(const float* x, unsigned n);", ("d3f_f", "n")),                     # a parameter type outside the map
    ("int d3f_f(const struct_t* x);", ("d3f_f", "x")),                              # ... a pointer to something unknown
    ("short d3f_f(int n);", ("d3f_f", "return type")),                               # a return type outside the map
    ("int d3f_a(int n)\nint d3f_b(int n);", ("d3f_a",)),                             # no ';': would hide d3f_a or d3f_b
    ("int d3f_a(int n);\nint d3f_b(int n)\n", ("d3f_b",)),
    ("int d3f_f(int (*callback)(int));", ("d3f_f",)),                                # not a plain parameter list
    ("int d3f_f(int n);\nint d3f_f(int n);", ("d3f_f",)),                            # declared twice
    ("#define D3F_CALL(x) d3f_f(x)\nint d3f_f(int n);", ("d3f_<name>(",)),           # a use no prototype accounts for
    ("static int helper(int n);", ("helper",)),                                      # a statement that is no d3f_ prototype
])
def test_the_parser_raises_on_prototypes_it_cannot_take(text, names):
    with pytest.raises(RuntimeError) as e:
        _native.parse_prototypes(text, {})
    for n in names:
        assert n in str(e.value), str(e.value)


@pytest.mark.parametrize("line", ["#define D3F_N sizeof(int)", "#define D3F_N ((float*)1)", "#define D3F_N 1.5",
                                  "#define D3F_N D3F_LATER\n#define D3F_LATER 1", "#define D3F_N", "#define D3F_N(x) 1"])
def test_the_parser_raises_on_a_define_that_is_no_integer(line):
    with pytest.raises(RuntimeError) as e:
        _native.parse_defines("#define D3F_ONE 1\n" + line)
    assert "D3F_N" in str(e.value)


def test_the_parser_on_synthetic_text():
    C = ctypes
    text = """/* int d3f_commented_out(int n); */
    #define D3F_A 3 /* three */
    #define D3F_B (D3F_A << 4)
    #define D3F_C (-(D3F_B | 0x1))
    #define D3F_SPACK_READY ((float*)(uintptr_t)1)
    typedef struct d3f_s {
      const float* p; /* [n] */
      int32_t n, m[3], k;
      double R[9], t[3];
      uint64_t key;
      void *a, *b;
    } d3f_s;
    const char* d3f_name(void);
    void d3f_take(const d3f_s* s, void* const* ptrs /* host */, int64_t n, const uint8_t* mask, char* out);
    """
    assert _native.parse_defines(text) == {"D3F_A": 3, "D3F_B": 48, "D3F_C": -49}
    fields = _native.parse_struct(text, "d3f_s")
    assert fields == [("p", C.c_void_p), ("n", C.c_int32), ("m", C.c_int32 * 3), ("k", C.c_int32), ("R", C.c_double * 9),
                      ("t", C.c_double * 3), ("key", C.c_uint64), ("a", C.c_void_p), ("b", C.c_void_p)]
    S = type("S", (C.Structure,), {"_fields_": fields})
    assert _native.parse_prototypes(text, {"d3f_s": S}) == {
        "d3f_name": (C.c_char_p, []),
        "d3f_take": (None, [C.POINTER(S), C.c_void_p, C.c_int64, C.c_void_p, C.c_char_p])}
    for bad in ("typedef struct d3f_s { long n; } d3f_s;", "typedef struct d3f_s { int32_t; } d3f_s;",
                "typedef struct d3f_other { int32_t n; } d3f_other;"):
        with pytest.raises(RuntimeError):
            _native.parse_struct(bad, "d3f_s")


def test_every_define_is_a_module_attribute():
    """An independent, crude list of the header's defines against what _native carries; ERRORS and STATUS_BITS by name."""
    src = open(os.path.join(REPO, "include", "d3feat_hip.h")).read()
    names = re.findall(r"^#define\s+(D3F_\w+)", src, flags=re.M)
    assert len(names) == len(set(names)) >= 55
    assert sorted(set(names) - {"D3F_SPACK_READY"}) == sorted(_native.DEFINES)
    assert not hasattr(_native, "D3F_SPACK_READY")
    for n, v in _native.DEFINES.items():
        assert type(v) is int and getattr(_native, n) == v
    assert (_native.D3F_EINVAL, _native.D3F_EWORKSPACE, _native.D3F_ELAUNCH) == (-1, -2, -3)
    assert _native.D3F_RANSAC_MAX_HYPOTHESES == 1 << 24 and _native.D3F_PG_MAX_EDGES == 1 << 20
    assert sorted(_native.ERRORS) == [-3, -2, -1]
    assert sorted(_native.STATUS_BITS) == [1, 2, 4, 8, 16, 32]
    assert _native.STATUS_BITS[_native.D3F_ST_TABLE_FULL] == "voxel hash table full"


def test_the_c_compiler_agrees_on_structs_and_defines(tmp_path):
    """Second witness: a C program that includes the header prints sizeof, every field's offsetof and size, and every
    integer define; the ctypes classes and _native.D3F_* must say the same."""
    cc = [shutil.which("cc")] if shutil.which("cc") else [shutil.which("hipcc"), "-x", "c++"]
    if not cc[0]:
        pytest.skip("no C compiler")
    lines, expected = [], []
    for cname, cls in _native.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        expected.append("%s %d" % (cname, ctypes.sizeof(cls)))
        for field, ctype in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (cname, field, cname, field, cname, field))
            expected.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, ctypes.sizeof(ctype)))
    for name, value in _native.DEFINES.items():
        lines.append('printf("%s %%lld\\n", (long long)(%s));' % (name, name))
        expected.append("%s %d" % (name, value))
    assert len(expected) == 3 + 11 + 12 + 14 + len(_native.DEFINES) and len(_native.DEFINES) >= 54   # fields per struct
    src = tmp_path / "witness.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "d3feat_hip.h"\nint main(void) {\n  %s\n  return 0;\n}\n'
                   % "\n  ".join(lines))
    exe = str(tmp_path / "witness")
    subprocess.check_call(cc + ["-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe]).decode().split("\n")[:-1] == expected


STARRED_CALL_SITES = ["d3f_depth_pyramid", "d3f_depth_pyramid_host", "d3f_detection_rows_backward",
                      "d3f_detection_rows_forward", "d3f_rgbd_pyramid", "d3f_rgbd_pyramid_host", "d3f_tsdf_sparse_mark",
                      "d3f_tsdf_sparse_mark_host"]


def test_every_call_site_passes_as_many_arguments_as_the_header_declares():
    """<expr>.d3f_<name>(...) anywhere in the package: the argument count is the prototype's.  A call with a starred
    argument cannot be counted; those are the eight listed above and no others."""
    counted, starred, wrong = 0, [], []
    for root, _, files in os.walk(os.path.dirname(_native.__file__)):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(root, f)
            for node in ast.walk(ast.parse(open(path).read(), path)):
                if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                        and node.func.attr.startswith("d3f_")):
                    continue
                name = node.func.attr
                if any(isinstance(a, ast.Starred) for a in node.args):
                    starred.append(name)
                    continue
                counted += 1
                if node.keywords or len(node.args) != len(_native.SIGNATURES[name][1]):
                    wrong.append("%s:%d %s passes %d of %d" % (os.path.relpath(path, REPO), node.lineno, name,
                                                              len(node.args), len(_native.SIGNATURES[name][1])))
    assert not wrong, wrong
    assert sorted(starred) == STARRED_CALL_SITES
    assert counted >= 138


def test_no_gpu_calls_needed_for_size_queries():
    lib = _native.lib()
    assert lib.d3f_version().decode().startswith("d3feat-hip")
    assert lib.d3f_radius_grid_ws_bytes(1000) > 0
    assert lib.d3f_grid_subsample_ws_bytes(1000, 2) > 0
    assert lib.d3f_kpconv_ws_bytes(100, 100, 40, 15, 32, 32) >= 2 * 100 * 15 * 32 * 4
    assert lib.d3f_circle_det_loss_stats_floats(128) == 6 * 128


def test_general_path_kpconv_entries_reject_bad_arguments_on_the_host():
    """d3f_kpconv_aggregate_modes / _grad_input_modes / _grad_input_modes_gather: a mode outside the table of
    kpconv_modes.hpp, K > 16, Cin > 512 or extent = 0 is D3F_EINVAL before anything touches a device (the addresses are
    never read); the gather entry also wants exactly one of the two forms of the transpose."""
    lib = _native.lib()
    p, nq, ns, h = 0x10000, 5, 4, 3         # (16-byte aligned, as the exact-form table has to be)

    def gather(mode=0, K=15, Cin=8, extent=0.1, csr=p, rel=None):
        return lib.d3f_kpconv_grad_input_modes_gather(p, nq, p, ns, csr, csr, rel, 7, Cin, p, K, extent, mode, p, p, None)

    def table_entries(mode=0, K=15, Cin=8, extent=0.1):
        return (lib.d3f_kpconv_aggregate_modes(p, nq, p, ns, p, h, p, Cin, p, K, extent, mode, p, p, None),
                lib.d3f_kpconv_grad_input_modes(p, nq, p, ns, p, h, Cin, p, K, extent, mode, p, p, None))
    # (every call below has exactly one bad argument, so none of them gets as far as a launch)
    for kw in [dict(mode=m) for m in (-1, 3, 7 + 1)] + [dict(K=17), dict(Cin=513), dict(extent=0.0)]:
        assert table_entries(**kw) + (gather(**kw),) == (_native.D3F_EINVAL,) * 3, kw
    assert gather(rel=p) == _native.D3F_EINVAL               # both forms of the transpose
    assert gather(csr=None) == _native.D3F_EINVAL            # neither


def test_tunables_struct_round_trips_and_rejects_nonsense():
    """d3f_get_tunables / d3f_set_tunables: the library's only knobs (it reads no environment); defaults are all zero."""
    lib = _native.lib()
    t = _native.Tunables()
    lib.d3f_get_tunables(ctypes.byref(t))
    names = [n for n, _ in _native.Tunables._fields_ if n != "reserved"]
    assert names == ["atb_task_us", "atb_form", "atb_first_form_wgs", "match_wgs", "agg_through_lds", "atb_pipe",
                     "xw_rows", "xw_split", "rowgemm_wide", "rowgemm_rt"]
    assert [getattr(t, n) for n in names] == [0] * len(names)
    assert ctypes.sizeof(t) == 64
    old = _native.set_tunables(atb_task_us=33, atb_form=2)
    lib.d3f_get_tunables(ctypes.byref(t))
    assert (t.atb_task_us, t.atb_form) == (33, 2)
    _native.set_tunables(**old)
    bad = _native.Tunables()
    bad.atb_form = 7
    assert lib.d3f_set_tunables(ctypes.byref(bad)) == -1
    for field, value in (("xw_rows", 5), ("xw_split", 65), ("rowgemm_wide", 3), ("rowgemm_rt", 2)):
        bad = _native.Tunables()
        setattr(bad, field, value)
        assert lib.d3f_set_tunables(ctypes.byref(bad)) == -1, field
    assert lib.d3f_set_tunables(None) == -1
    lib.d3f_get_tunables(ctypes.byref(t))
    assert (t.atb_task_us, t.atb_form) == (0, 0)


def test_gemm_epilogue_support_and_workspace_are_host_computations():
    """d3f_gemm_epilogue_supported / _ws_bytes need no GPU: multiples of 16, the block form only for reduction-contiguous
    weights in blocks of 64; a split reduction (few rows against a long reduction) asks for its slabs."""
    lib = _native.lib()
    assert lib.d3f_gemm_epilogue_supported(512, 7680, 512, 1, 0) == 1
    assert lib.d3f_gemm_epilogue_supported(1792, 3840, 256, 0, 256) == 1
    assert lib.d3f_gemm_epilogue_supported(1792, 3840, 256, 1, 256) == 0
    assert lib.d3f_gemm_epilogue_supported(1792, 3840, 250, 0, 0) == 0
    assert lib.d3f_gemm_epilogue_supported(0, 64, 64, 0, 0) == 0
    assert lib.d3f_gemm_epilogue_ws_bytes(512, 7680, 512) >= 8 * 512 * 512 * 4       # 8 partitions of the reduction
    assert lib.d3f_gemm_epilogue_ws_bytes(114624, 128, 32) == 256                      # undivided: no slabs
    old = _native.set_tunables(xw_split=1)
    try:
        assert lib.d3f_gemm_epilogue_ws_bytes(512, 7680, 512) == 256
    finally:
        _native.set_tunables(**old)


def test_grouped_weight_gradient_plan_is_a_host_computation():
    """d3f_linear_grad_weight_group_ws_bytes needs no GPU: slab bytes of a queue; few rows against a large aligned target
    take no slab at all (undivided reduction written straight to the target); unsupported widths give 0."""
    lib = _native.lib()
    arr = (_native.AtbProblem * 2)()
    for q, (n, cin, cout) in zip(arr, ((114688, 32, 128), (512, 512, 7680))):
        q.x, q.grad_out, q.grad_w = 0x10000, 0x20000, 0x30000       # (addresses are only checked for alignment here)
        q.N, q.Cin, q.Cout, q.ldw = n, cin, cout, cin
    both = lib.d3f_linear_grad_weight_group_ws_bytes(arr, 2)
    first = lib.d3f_linear_grad_weight_group_ws_bytes(arr, 1)
    assert first > 256 and (first - 256) % (128 * 32 * 4) == 0     # whole slabs of the 128 x 32 gradient
    assert both == first                                            # the direct problem adds nothing
    arr[1].grad_w = 0x30004                                         # not 16-byte aligned: partitions + slabs after all
    assert lib.d3f_linear_grad_weight_group_ws_bytes(arr, 2) >= first + 8 * 7680 * 512 * 4
    arr[1].Cin = 24
    assert lib.d3f_linear_grad_weight_group_ws_bytes(arr, 2) == 0
    assert lib.d3f_linear_grad_weight_group_ws_bytes(None, 2) == 0
