"""Inputs of a landmark segment with chosen inverted frames, shared by the CPU and GPU tests of ``segment_assemble``."""
import numpy as np


def segment_inputs(T, inverted):
    """dis, base, fid such that the assembled inner-lip polygon (points 60 .. 67) is a counter-clockwise octagon of area ~0.05
    in every frame, mirrored in y (area ~-0.05) in the frames of ``inverted``."""
    rs = np.random.RandomState(T)
    fid = (rs.randn(68, 3) * 0.2).astype(np.float32)
    ang = 2 * np.pi * np.arange(8) / 8
    fid[60:68, 0], fid[60:68, 1] = 0.2 * np.cos(ang), 0.1 * np.sin(ang)
    dis = (rs.randn(T, 204) * 0.01).astype(np.float32)
    base = (rs.randn(T, 68, 3) * 0.01).astype(np.float32)
    for j in inverted:
        base[j, 60:68, 1] -= 2 * fid[60:68, 1]
    return dis, base.reshape(T, 204), fid.reshape(1, 204)
