"""A SHA-256 of everything the public TSDF integrate and ray-cast functions return, for comparing two trees: the script
uses ``ops.tsdf_*`` alone, so the same text runs in either, and the two lists of hashes must be equal line for line.

Inputs: the small cases of tests/tsdf_scene.py and the brick-face volume, the batch of tests/tsdf_sparse_cases.py whose
middle volume owns no frame, and the two fragments of the room.  For each: uint16 and f32 depth; Cc 0, 1 and 3; the
whole call and the call split in two with ``into=`` (every volume's first half of its frames, rounded up, then the
rest: a volume of one frame owns none in the second call); dense and sparse; ray-casts of two views per volume without
and with normals (and the colour image when Cc > 0), and a ray-cast of no view.

    python profiles/tsdf_entry_fold_identity.py [--device] [--out FILE]

Without --device the host twins run and no GPU is needed."""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import tsdf_sparse_cases as SC  # noqa: E402
from d3feat_pytorch_amd import ops  # noqa: E402


def digest(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a))
    return "%s%s %s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()[:24])


def colour_frames(shape, channels):
    """f32 intensity [F,H,W] for one channel, uint8 RGB [F,H,W,3] for three, None for none."""
    rng = np.random.RandomState(7)
    if channels == 1:
        return rng.uniform(0.0, 1.0, shape).astype(np.float32)
    return rng.randint(0, 256, tuple(shape) + (3,)).astype(np.uint8) if channels == 3 else None


def halves(frame_start):
    """(frames, frame_start) of the two calls of a split: each volume's first half, rounded up, then the rest."""
    out = []
    for part in (0, 1):
        frames, starts = [], [0]
        for f0, f1 in zip(frame_start, frame_start[1:]):
            k = f0 + (f1 - f0 + 1) // 2
            frames += list(range(f0, k)) if part == 0 else list(range(k, f1))
            starts.append(len(frames))
        out.append((frames, starts))
    return out


def run(suffix, say):
    fn = {stem: getattr(ops, stem + suffix) for stem in ("tsdf_integrate", "tsdf_allocate", "tsdf_integrate_sparse",
                                                         "tsdf_raycast", "tsdf_raycast_sparse")}
    cases = dict(SC.cases())
    cases['batch_zero_frames'] = SC.batch_of(SC.EMPTY_BETWEEN['zero_frames'])
    cases['room'] = SC.room_args()
    for name, case in cases.items():
        fs = [int(x) for x in case['frame_start']]
        M, C = np.asarray(case['volume_to_camera']), np.asarray(case['camera_to_volume'])
        volume = (case['origin'], case['dims'], case['voxel'])
        rest = (case['trunc'], case['depth_scale'], case['depth_max'])
        views = [f for f0, f1 in zip(fs, fs[1:]) for f in range(f0, min(f0 + 2, f1))]
        view_volume = [v for v, (f0, f1) in enumerate(zip(fs, fs[1:])) for _ in range(f0, min(f0 + 2, f1))]
        for f32 in (False, True):
            depth = np.asarray(case['depth'])
            if f32 and depth.dtype == np.uint16:
                depth = depth.astype(np.float32) / np.float32(1000.0)
            H, W = depth.shape[1:]
            sv = fn["tsdf_allocate"](depth, fs, case['intrinsics'], C, *volume, *rest)
            say("%s %s tables" % (name, depth.dtype), sv.brick_index, sv.brick_coord, sv.brick_start)
            for Cc in (0, 1, 3):
                colour = colour_frames(depth.shape, Cc)
                tag = "%s %s Cc=%d" % (name, depth.dtype, Cc)

                def fuse(sparse, frames, starts, into):
                    kw = dict(into=into)
                    if Cc:
                        kw['color'] = colour[frames]
                    if sparse:
                        return fn["tsdf_integrate_sparse"](depth[frames], starts, case['intrinsics'], M[frames], sv,
                                                           *rest, **kw)
                    out = fn["tsdf_integrate"](depth[frames], starts, case['intrinsics'], M[frames], *volume, *rest,
                                               **kw)
                    return (out[0], out[1]) + tuple(out[3:])                  # without vol_start

                for sparse in (False, True):
                    kind = "sparse" if sparse else "dense"
                    whole = fuse(sparse, list(range(depth.shape[0])), fs, None)
                    say("%s %s whole" % (tag, kind), *whole)
                    (first, s1), (second, s2) = halves(fs)
                    split = fuse(sparse, second, s2, fuse(sparse, first, s1, None))
                    say("%s %s split" % (tag, kind), *split)
                    model = (whole[0], whole[1], sv) if sparse else (whole[0], whole[1], out_start(case), *volume)
                    cast = fn["tsdf_raycast_sparse" if sparse else "tsdf_raycast"]
                    col = dict(color=whole[2]) if Cc else {}
                    for normals in (False, True):
                        out = cast(*model, case['trunc'], case['intrinsics'], C[views], H, W, view_volume=view_volume,
                                   normals=normals, **col)
                        say("%s %s cast normals=%d" % (tag, kind, normals),
                            *(out if isinstance(out, tuple) else (out,)))
                    out = cast(*model, case['trunc'], case['intrinsics'], C[:0], H, W, view_volume=[], normals=True,
                               **col)
                    say("%s %s cast R=0" % (tag, kind), *out)


def out_start(case):
    dims = np.asarray(case['dims'], dtype=np.int64).reshape(-1, 3)
    return np.concatenate([[0], np.cumsum(dims.prod(axis=1))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="the kernels instead of the host twins")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    lines = []

    def say(label, *arrays):
        for j, a in enumerate(arrays):
            lines.append("%s [%d] %s" % (label, j, digest(a)))
    run("" if opt.device else "_host", say)
    lines.append("%d outputs, all: %s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
    text = "\n".join(lines) + "\n"
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(text)
    print(text if not opt.out else lines[-1])


if __name__ == "__main__":
    main()
