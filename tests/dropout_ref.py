"""numpy restatement of the seeded Dropout2d masks (rgbmanip_amd/csrc/dropout.hip, DESIGN.md "Seeded Dropout2d")."""
import numpy as np

PER_VIEW = 256 + 64          # up_1's channels, then up_2's
_M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def threshold(p):
    return int(round(float(np.float32(p)) * 16777216.0))


def scale(p):
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_bits(seed, pose, view, site, channel):
    """the 24-bit uniform of each (pose, view, site, channel): broadcasting uint64 arrays"""
    key = (np.asarray(pose, np.uint64) << np.uint64(10)) | (np.asarray(view, np.uint64) << np.uint64(9)) | \
          (np.asarray(site, np.uint64) << np.uint64(8)) | np.asarray(channel, np.uint64)
    sm = mix64(np.uint64(int(seed) & _M64))
    with np.errstate(over="ignore"):
        z = mix64(sm + key * np.uint64(0x9E3779B97F4A7C15))
    return (z >> np.uint64(40)).astype(np.uint32)


def masks(p, seed, B, first_pose=0):
    """[2B, 320] fp32 factors of a forward of B poses whose first pose has global index `first_pose` (rows: the view-1 crops of the
    batch, then the view-2 crops; columns: up_1's 256 channels, then up_2's 64)"""
    v = np.arange(2 * B)[:, None]
    r = np.arange(PER_VIEW)[None, :]
    view = v // B
    site = (r >= 256).astype(np.int64)
    u = keep_bits(seed, first_pose + v - view * B, view, site, r - 256 * site)
    return np.where(u >= threshold(p), scale(p), np.float32(0)).astype(np.float32)
