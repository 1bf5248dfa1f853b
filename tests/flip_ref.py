"""The flip test's arithmetic in numpy, as include/simple_pose_hip.h states it: the yardstick of tests/test_gpu_flip.py.

    f[b,j,y,x]   = hm_flipped[b, perm[j], y, w-1-x]
    g[b,j,y,x]   = shift ? (x >= 1 ? f[b,j,y,x-1] : f[b,j,y,0]) : f[b,j,y,x]
    out[b,j,y,x] = (hm[b,j,y,x] + g[b,j,y,x]) * 0.5f

numpy rounds every float32 operation once (one add, one multiply) and keeps denormals, as the kernel does: comparisons are bitwise."""
import numpy as np


def perm_of(joint_pairs, num_joints):
    perm = np.arange(num_joints)
    for a, b in joint_pairs:
        perm[a], perm[b] = b, a
    return perm


def mirror_w(a):
    """dst[..., x] = src[..., w-1-x] for fp32 [..., w]; uint8 pixels [..., w, 3] mirror along w, the three bytes of a pixel stay in order."""
    a = np.asarray(a)
    return (a[..., ::-1, :] if a.dtype == np.uint8 else a[..., ::-1]).copy()


def merge_flipped(hm, hm_flipped, joint_pairs, shift=False):
    hm, hm_flipped = np.asarray(hm, np.float32), np.asarray(hm_flipped, np.float32)
    f = hm_flipped[:, perm_of(joint_pairs, hm.shape[1])][..., ::-1]
    g = f
    if shift:
        g = f.copy()
        g[..., 1:] = f[..., :-1]                                 # flipped[..., 1:] = flipped.clone()[..., :-1]; column 0 stays f[..., 0]
    out = (hm + g) * np.float32(0.5)
    assert out.dtype == np.float32
    return out


def flipped_twin(hm, joint_pairs):
    """The hm_flipped for which the merge (shift off) gives hm back: the exact mirror + pair swap of hm."""
    hm = np.asarray(hm, np.float32)
    return hm[:, perm_of(joint_pairs, hm.shape[1])][..., ::-1].copy()                   # the pair swap is an involution
