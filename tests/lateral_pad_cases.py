"""Meshes shared by tests/test_lateral_pad.py and tests/test_gpu_lateral_pad.py: what the lists' lateral bound (dxv_dirmap.h:
dm_lateral_pad) must fall back on -- slivers, and triangles seen edge-on from the grid's centre."""
import numpy as np


def _mesh(pos):
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    nrm = pos / np.maximum(np.linalg.norm(pos, axis=1), 1e-30)[:, None]
    pins = np.array([[-1, -1, -1, 0, 0, 1], [1, 1, 1, 0, 0, 1]], np.float32)
    return np.concatenate([np.hstack([pos, nrm]).astype(np.float32), pins]).astype(np.float32), np.arange(len(pos), dtype=np.uint32)


def sliver_mesh(rng, n=160):
    """long triangles of altitude 1e-8 .. 1e-3 of their length, scattered round the centre; and a strip of ever thinner ones side by side"""
    tris = []
    for _ in range(n):
        a = rng.uniform(-0.8, 0.8, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        b = np.clip(a + rng.uniform(0.1, 0.9) * d, -1, 1)
        p = np.cross(b - a, rng.normal(size=3))
        p /= max(np.linalg.norm(p), 1e-30)
        c = a + rng.uniform(0, 1) * (b - a) + p * np.linalg.norm(b - a) * 10.0 ** rng.uniform(-8, -3)
        tris.append([a, b, np.clip(c, -1, 1)])
    x = -0.6
    for k in range(24):                                                 # a fan of slivers in the plane z = 0.55, sharing long edges
        w = 0.05 * 0.6 ** k
        tris.append([[x, -0.7, 0.55], [x + w, 0.7, 0.55], [x, 0.7, 0.55]])
        tris.append([[x, -0.7, 0.55], [x + w, -0.7, 0.55], [x + w, 0.7, 0.55]])
        x += w
    return _mesh(tris)


def grazing_fan(rng, n=96):
    """triangles that all contain (nearly) a line through the centre: their planes turn about the ray direction d like the pages of a book,
    tilted out of it by 1e-6 .. 1e-2 -- every ray along d sees them edge-on"""
    tris = []
    for k in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        t1 = np.cross(d, rng.normal(size=3))
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(d, t1)
        eps = 10.0 ** rng.uniform(-6, -2) * rng.choice((-1, 1))
        e1 = np.cos(eps) * d - np.sin(eps) * t2
        c = d * rng.uniform(0.3, 0.6)
        s = rng.uniform(0.05, 0.3)
        tris.append([np.clip(c + s * (rng.uniform(-1, 1) * e1 + rng.uniform(-1, 1) * t1), -1, 1) for _ in range(3)])
    return _mesh(tris)
