"""The voxel occupancy counts of r2dm_amd.geometry in plain numpy, and again in plain Python sets for tiny inputs.

The voxel of a point at size s is ``floor(x / s)`` per axis with ``x`` and ``s`` float32 and the division an IEEE float32 division, which
is what numpy's ``/`` on float32 operands is.  Everything after that is integers."""
import numpy as np

HALF = 1 << 20


def voxels(points, size):
    """(n,>=3) points -> (n,3) int64 voxel indices; every point must be finite and inside the grid"""
    p = np.asarray(points, dtype=np.float32)[:, :3]
    v = np.floor(p / np.float32(size))
    assert np.isfinite(v).all() and (v >= -HALF).all() and (v < HALF).all()
    return v.astype(np.int64)


def keys(points, size):
    """the three biased 21-bit indices packed into one int64 per point"""
    v = voxels(points, size) + HALF
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def occupancy(member_clouds, target_cloud, size):
    """K member clouds and a target -> (member (K,2) = |V(M_k)|, |V(M_k) n V(T)|; hist (2,K+1) = #{voxels of the union: o, c}) int64"""
    K = len(member_clouds)
    sets = [np.unique(keys(c, size)) for c in member_clouds]
    tset = np.unique(keys(target_cloud, size))
    union = np.unique(np.concatenate(sets + [tset]))
    c = np.zeros(union.size, np.int64)
    for s in sets:
        c += np.isin(union, s)
    o = np.isin(union, tset).astype(np.int64)
    hist = np.bincount(o * (K + 1) + c, minlength=2 * (K + 1)).reshape(2, K + 1).astype(np.int64)
    member = np.array([[s.size, np.isin(s, tset).sum()] for s in sets], np.int64).reshape(K, 2)
    return member, hist


def occupancy_groups(a, off_a, b, off_b, members, targets, sizes):
    """the outputs of ``voxel_occupancy_counts``: member (G,S,K,2), hist (G,S,2,K+1)"""
    a, b = np.asarray(a), np.asarray(b)
    cloud = lambda p, off, i: p[int(off[i]):int(off[i + 1])]
    G, K = np.asarray(members).shape
    member, hist = np.zeros((G, len(sizes), K, 2), np.int64), np.zeros((G, len(sizes), 2, K + 1), np.int64)
    for g in range(G):
        for s, size in enumerate(sizes):
            member[g, s], hist[g, s] = occupancy([cloud(a, off_a, k) for k in members[g]], cloud(b, off_b, targets[g]), size)
    return member, hist


def iou_counts(a, b, size):
    """[intersection, voxels_a, voxels_b] of two clouds"""
    ka, kb = np.unique(keys(a, size)), np.unique(keys(b, size))
    return np.array([np.intersect1d(ka, kb).size, ka.size, kb.size], np.int64)


# ---- the same with Python sets of tuples (tiny inputs) ---------------------------------------------------------------------------------------
def voxel_set(points, size):
    s = np.float32(size)
    return {tuple(int(np.floor(np.float32(x) / s)) for x in p[:3]) for p in np.asarray(points, dtype=np.float32)}


def occupancy_sets(member_clouds, target_cloud, size):
    K = len(member_clouds)
    sets, tset = [voxel_set(c, size) for c in member_clouds], voxel_set(target_cloud, size)
    union = set().union(tset, *sets)
    hist = np.zeros((2, K + 1), np.int64)
    for v in union:
        hist[int(v in tset), sum(v in s for s in sets)] += 1
    member = np.array([[len(s), len(s & tset)] for s in sets], np.int64).reshape(K, 2)
    return member, hist
