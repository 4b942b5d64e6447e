"""Frames, the independent composition and the comparisons that tests/test_scene_memory_flow_cpu.py and
tests/test_gpu_scene_memory_flow.py share: memory and velocities in one depth call (include/omds.h: omds_depth_scene_memory_flow).

``compose`` restates the definition WITHOUT calling it: the words are those of the host definition of the scene memory
(engine.depth_scene_memory), the points those of engine.depth_points, the velocities, labels and flags on the seen sublist T those of
engine.point_cloud_flow / point_cloud_object_flow, and step 4 (a remembered sphere, and a seen one whose stored word was >= 2, stands
still) is numpy.  The matched flag of a sphere, which the host definitions of the flow only return summed, is restated from its
meaning: some occupied cell of the previous frame lies within ``reach`` cells."""
import numpy as np

import scene_memory_cases as sm
from cloud_cases import F32, cells_of

KEYS = ("words", "counts", "spheres", "vel", "age", "label", "object", "n_matched", "n_objects", "n_objects_matched")


def obj_of(link=1, min_cells=4):
    from optimalmodulationds_amd.engine import cloud_object_spec
    return cloud_object_spec(link, min_cells)


def points_of(cams, images, filt=None):
    from optimalmodulationds_amd.engine import depth_points
    if images is None:
        return np.zeros((0, 3), F32)
    return np.concatenate([depth_points(im, c, filter=filt)[0] for c, im in zip(cams, images)]).astype(F32)


def occupied_cells(spec, pts):
    from optimalmodulationds_amd.engine import point_cloud_spheres
    return cells_of(spec, point_cloud_spheres(pts, spec, cap=65536)) if len(pts) else np.zeros(0, np.int64)


def within_reach(spec, cells, others, reach):
    """[len(cells)] bool: some cell of ``others`` lies within ``reach`` cells (each axis) of the cell"""
    dims = np.array(list(spec.dims), np.int64)
    idx = lambda c: np.stack([c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])], 1)
    a, b = idx(np.asarray(cells, np.int64)), idx(np.asarray(others, np.int64))
    if not len(a) or not len(b):
        return np.zeros(len(a), bool)
    return (np.abs(a[:, None, :] - b[None, :, :]).max(2) <= reach).any(1)


def compose(spec, mem, track, obj, cams, images, prev_images, m_in, keep_now=None, filt=None):
    """the definition's outputs (the dict of engine.depth_scene_memory_flow) composed from the three existing host definitions"""
    from optimalmodulationds_amd.engine import depth_scene_memory, point_cloud_flow, point_cloud_object_flow
    words, counts = depth_scene_memory(images, cams, spec, mem, m_in, filter=filt)
    words = words.copy()
    cand = np.nonzero(words)[0]
    keep = np.ones(len(cand), bool) if keep_now is None else np.asarray(keep_now, bool)
    words[cand[~keep]] = 0
    final = cand[keep]
    now, prev = points_of(cams, images, filt), points_of(cams, prev_images, filt)
    occ = occupied_cells(spec, now)
    in_final = np.isin(occ, final)
    seen = occ[in_final]                                   # T, in cell order
    stored = np.zeros(sm.n_cells_of(spec), np.uint32) if m_in is None else np.asarray(m_in, np.uint32)
    have_prev = prev_images is not None
    t_vel, t_label, t_object = np.zeros((len(seen), 3), F32), np.full(len(seen), -1, np.int32), np.zeros(len(seen), np.int32)
    n_objects, n_accepted = 0, -1
    if obj is not None:
        _, vel, label, flag, _, n_objects, n_acc = point_cloud_object_flow(prev, now, spec, track, obj, keep_now=in_final, cap=65536)
        t_label = label
        if have_prev:
            t_vel, t_object, n_accepted = vel, flag, n_acc
    elif have_prev:
        t_vel = point_cloud_flow(prev, now, spec, track, cap=65536)[1][in_final]
    t_matched = (within_reach(spec, seen, occupied_cells(spec, prev), int(track.reach)) | (t_object != 0)) if have_prev else np.zeros(len(seen), bool)
    at = np.searchsorted(final, seen)                      # T's places in the final list
    n = len(final)
    vel, label, flag, matched = np.zeros((n, 3), F32), np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, bool)
    moves = stored[seen] < 2                               # step 4 on T; outside T nothing was measured
    vel[at[moves]], flag[at[moves]], matched[at[moves]] = t_vel[moves], t_object[moves], t_matched[moves]
    label[at] = t_label
    radius = F32(spec.radius) if spec.radius > 0 else F32(0.8660254) * F32(spec.voxel)
    spheres = np.concatenate([sm.centres_of(spec, final), np.full((n, 1), radius, F32)], 1).astype(F32)
    return dict(words=words, counts=counts + (int((~keep).sum()),), spheres=spheres, vel=vel, age=(words[final].astype(np.int64) - 1).astype(np.int32),
                label=label, object=flag, n_matched=int(matched.sum()) if have_prev else -1, n_objects=n_objects, n_objects_matched=n_accepted,
                seen=at, stored=stored[final])


def same(got, want, what=""):
    """every output of the definition as bits"""
    for key in KEYS:
        a, b = got[key], want[key]
        if isinstance(a, np.ndarray) and a.dtype == np.float32:
            a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32)
        assert np.array_equal(a, b), f"{what}: {key} differs"


# ---- the crossing plate --------------------------------------------------------------------------------------------------------------
CROSS_MARGIN = 0.25          # the explicit clear_margin: the wall's return, 1 m behind the plate's cells, clears them


def crossing(cam, n=4, first=9, width=16, step=8, wall=2.0, plate=1.0):
    """``n`` frames of the exact camera (64 columns wide): a plate at 1 m over the columns [first + step t, first + step t + width) in
    front of a wall at 2 m.  At 1 m a cell of GRID_SMALL is exactly 8 columns [9 + 8 j, 17 + 8 j): the plate moves one voxel per frame
    towards -y and covers the same pixels of every cell it is in"""
    w = sm.frame(cam, wall, 2)
    return [sm.put(w, cam, plate, slice(None), slice(first + step * t, first + step * t + width)) for t in range(n)]
