"""The sampler and the winner rule that the RANSAC stages share (photogrammetry_amd/csrc/pgx_ransac.h), restated once for the
yardsticks: pose_ref.py, register_ref.py and verify_ref.py import from here (oracle/pose_np.py keeps its own copy, oracle/
does not import from tests/).  tests/test_ransac_ref.py pins literal draws of all three stages."""
M64 = (1 << 64) - 1
STREAM_MUL = 0xD1B54A32D192ED03


def splitmix64(state):
    """-> (new state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def stream_seed(seed, hi, s):
    """The state of the stream of sample s of row `hi` (an image pair, a frame) under `seed`.  It is also the seed under which
    row 0 / sample 0 of a call runs that stream."""
    return (seed ^ ((hi & 0xFFFFFFFF) << 32) ^ (((s & 0xFFFFFFFF) * STREAM_MUL) & M64)) & M64


def draw(state, n, count):
    """`count` distinct positions of an n-entry list: each the stream's next output modulo n that is not yet taken"""
    ids = []
    while len(ids) < count:
        state, z = splitmix64(state)
        c = z % n
        if c not in ids:
            ids.append(c)
    return ids


def key(valid, count, index):
    """The key of a sample; the largest wins: most inliers first, then the smallest index; 0 means none"""
    return ((count + 1) << 32) | (0xFFFFFFFF - index) if valid else 0


def key_index(k):
    return 0xFFFFFFFF - (k & 0xFFFFFFFF)


def key_count(k):
    return (k >> 32) - 1
