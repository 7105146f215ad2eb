"""The two geometry rules of the users of ops.resize_u8 (evaluate.py --anchor_scales, decompress.py --max_side), shared with the tests."""


def reduced_size(H, W, r):
    """the size an H x W image is coded at by the anchor of scale r: (ceil(H / r), ceil(W / r))"""
    H, W, r = int(H), int(W), int(r)
    if H < 1 or W < 1 or r < 1:
        raise ValueError("reduced_size needs H, W, r >= 1")
    return -(-H // r), -(-W // r)


def max_side_size(H, W, N):
    """(H, W) if neither side exceeds N; else the longer side becomes N and the other keeps the aspect ratio, rounded half up,
    at least 1"""
    H, W, N = int(H), int(W), int(N)
    if H < 1 or W < 1 or N < 1:
        raise ValueError("max_side_size needs H, W, N >= 1")
    if max(H, W) <= N:
        return H, W
    if H >= W:
        return N, max(1, (2 * W * N + H) // (2 * H))
    return max(1, (2 * H * N + W) // (2 * W)), N
