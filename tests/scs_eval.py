"""A deterministic stand-in evaluator for SCS search tests: (post-softmax probabilities, value)
as a pure function of the state image.  Used on both sides of every comparison (reference,
oracle, device), so no network arithmetic is involved."""
import math

import numpy as np


def checksum_weights(n):
    i = np.arange(n, dtype=np.int64)
    return ((i * 2654435761) % 1000003).astype(np.float64) / 1000003.0


_W = {}


def _checksum(img):
    flat = np.asarray(img, np.float32).reshape(-1)
    w = _W.get(flat.size)
    if w is None:
        w = _W[flat.size] = checksum_weights(flat.size)
    return float(np.sum(flat.astype(np.float64) * w))


def evaluate_image_peaked(img, num_actions):
    """As evaluate_image, for searches that must go deep: a tie-free ranking of the actions whose best legal one
    clearly dominates (p[a] = exp(-80 frac((a + k) golden ratio)); the smallest is about e^-80, a normal float32) and a
    near-constant positive value -- SCS never negates Q, so the line visited so far keeps being followed."""
    s = _checksum(img)
    k = int(abs(s) * 977.0) % 19
    x = (np.arange(num_actions, dtype=np.float64) + k) * 0.6180339887498949
    p = np.exp(-80.0 * (x - np.floor(x))).astype(np.float32)
    p = p / np.sum(p)
    return p, np.float32(0.9 + 0.01 * math.sin(s))


def evaluate_image(img, num_actions):
    """img: float32 [C, R, Cc] -> (probs float32 [num_actions], value np.float32)."""
    s = _checksum(img)
    k = int(abs(s) * 977.0) % 17
    p = (1.0 + ((np.arange(num_actions, dtype=np.int64) * 31 + k) % 17)).astype(np.float32)
    p = p / np.sum(p)
    return p, np.float32(math.sin(s))
