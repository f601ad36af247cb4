"""The binding read from include/d3feat_hip.h against the hand-written one of an earlier commit (CPU only):

    python profiles/abi_header_identity.py [rev]          (rev defaults to HEAD~1: the commit before the change)

loads `git show rev:d3feat.pytorch_amd/_native.py` and `rev:.../ops.py` next to the working tree's modules and compares
every prototype, the three struct layouts, the error / status tables and every upper-case constant of ops.py; then the
code-line counts of the three files and the time of importing _native.py alone, median of fresh processes."""
import ctypes
import importlib.util
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FILES = ["d3feat.pytorch_amd/_native.py", "d3feat.pytorch_amd/ops.py", "tests/test_abi.py"]


def show(rev, path):
    return subprocess.check_output(["git", "-C", REPO, "show", "%s:%s" % (rev, path)]).decode()


def load(name, source, tmp):
    path = os.path.join(tmp, name.rsplit(".", 1)[-1] + ".py")
    with open(path, "w") as f:
        f.write(source)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plain(t):
    """A ctypes type as something comparable across two modules: POINTER(Tunables) of either module is ('*', fields)."""
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return ("*", plain(t._type_))
    if isinstance(t, type) and issubclass(t, ctypes.Structure):
        return [(n, plain(f)) for n, f in t._fields_]
    return t


def code_lines(source):
    return sum(1 for line in source.split("\n") if line.strip() and not line.strip().startswith("#"))


def import_ms(path, runs=9):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        subprocess.check_call([sys.executable, "-c", "import importlib.util as u; s = u.spec_from_file_location('n', %r); "
                               "m = u.module_from_spec(s); s.loader.exec_module(m)" % path])
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    print("parent = %s" % subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", rev]).decode().strip())
    import d3feat_pytorch_amd
    from d3feat_pytorch_amd import _native as new, ops as new_ops
    with tempfile.TemporaryDirectory() as tmp:
        old = load("parent_native", show(rev, FILES[0]), tmp)
        old_ops = load(d3feat_pytorch_amd.__name__ + ".parent_ops", show(rev, FILES[1]), tmp)
        diffs = 0
        for name in sorted(set(old.SIGNATURES) | set(new.SIGNATURES)):
            a, b = old.SIGNATURES.get(name), new.SIGNATURES.get(name)
            if a is None or b is None or (plain(a[0]), [plain(t) for t in a[1]]) != (plain(b[0]), [plain(t) for t in b[1]]):
                diffs += 1
                print("  DIFFERENT %s: %r -> %r" % (name, a, b))
        print("prototypes: %d in the parent's table, %d read from the header, %d arguments in all: %d differences"
              % (len(old.SIGNATURES), len(new.SIGNATURES), sum(len(a) for _, a in new.SIGNATURES.values()), diffs))
        for cls in ("Tunables", "AtbProblem", "AugmentJob"):
            a, b = getattr(old, cls), getattr(new, cls)
            same = plain(a) == plain(b) and ctypes.sizeof(a) == ctypes.sizeof(b) and a.__doc__ == b.__doc__ \
                and [getattr(a, n).offset for n, _ in a._fields_] == [getattr(b, n).offset for n, _ in b._fields_]
            diffs += not same
            print("struct %-10s %2d fields, %3d bytes: names, types, order, offsets, size and docstring %s"
                  % (cls, len(b._fields_), ctypes.sizeof(b), "equal" if same else "DIFFERENT"))
        for table in ("ERRORS", "STATUS_BITS"):
            same = getattr(old, table) == getattr(new, table)
            diffs += not same
            print("%-11s %d entries, keys and messages %s" % (table, len(getattr(new, table)), "equal" if same else "DIFFERENT"))
        names = [n for n in dir(old_ops) if n.isupper() and isinstance(getattr(old_ops, n), (int, float, tuple, dict))]
        names.append("_RGBD_KINDS")
        bad = [n for n in names if getattr(old_ops, n) != getattr(new_ops, n, None)
               or type(getattr(old_ops, n)) is not type(getattr(new_ops, n, None))]
        from_header = [n for n in names if isinstance(getattr(new_ops, n), int)
                       and new.DEFINES.get("D3F_" + n) == getattr(new_ops, n)]
        diffs += len(bad) + (sorted(set(dir(old_ops)) ^ set(dir(new_ops))) != [])
        print("ops.py: %d upper-case constants (%d carry a header name, + the 3 values of _RGBD_KINDS), same module names: "
              "%d differ %s" % (len(names), len(from_header), len(bad), bad or ""))
        print("defines: %d integer #define D3F_* are attributes of _native (D3F_SPACK_READY, a pointer cast, is not)"
              % len(new.DEFINES))
        print("%d differences" % diffs)
        print()
        print("code lines (not blank, not a comment line)     parent  change")
        for path in FILES:
            print("  %-44s %6d  %6d" % (path, code_lines(show(rev, path)), code_lines(open(os.path.join(REPO, path)).read())))
        print()
        # the parent's module reads no file and is timed where it was written out; the change's in place, next to the header
        m_old, m_new = import_ms(os.path.join(tmp, "parent_native.py")), import_ms(os.path.join(REPO, FILES[0]))
        open(os.path.join(tmp, "empty.py"), "w").close()
        base = import_ms(os.path.join(tmp, "empty.py"))
    print("import of _native.py alone, fresh process, median of 9 (min .. max), ms")
    print("  empty module  %6.1f (%5.1f .. %5.1f)" % base)
    print("  parent        %6.1f (%5.1f .. %5.1f)" % m_old)
    print("  change        %6.1f (%5.1f .. %5.1f)" % m_new)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
