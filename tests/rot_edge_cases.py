"""Edge-value inputs of the randomized Hadamard rotation (tests/rot_model.py); numpy only.  tests/test_rot_edge_cases_cpu.py proves on the model
that they do what they claim and that each of a list of wrong rotations changes the result of at least one of them;
tests/test_gpu_grouped_rotated_edges.py runs them on the device.

cases(G, seed, dt) -> {name: tensor of type dt}: float32 values, or bfloat16 bit patterns (uint16) built from bfloat16-representable values, never
by rounding.  Every tensor is whole groups of G followed by a ragged tail of G - 1 elements, the front of its own group 0 (a ragged group is not
rotated: a kernel that pads and rotates it shows).  d = rot_model.signs(G, seed), c = rot_model.scale_const(G).

  zeros         four groups: all +0.0; all -0.0; alternating +0.0, -0.0; -0.0 exactly where d is -1, so that d x is all +0.0.  The sign of a zero
                is observable: a + b of two zeros of unlike sign is +0.0, a - a is +0.0, -0.0 - (+0.0) is -0.0
  denormal_in   three groups, every element a nonzero denormal of the tensor's type: float32 N(0, 1) 1e-41 (an exact zero replaced by the
                smallest denormal), bfloat16 +-m 2^-133 with m in [1, 127]
  denormal_out  three groups of normal numbers +-[1, 2) 2^-124: c fwht(d x) is about N(0, 1) 2^-124, a fifth of it below 2^-126
  cancel        twelve groups of constant magnitude v in {3.25, 2^-126, 2^100}, four each: all +v; alternating +v, -v; v d (d x is the constant
                v: one sum of G v, zeros elsewhere); random signs.  Butterflies cancel exactly to zeros of either sign
  overflow      four groups.  (2.5 2^127 / G) d: d x is constant and the sums double every stage, 1.25 2^127 before the last one and past the
                largest float32 in it: one +inf, zeros elsewhere, no NaN.  (0.99 2^127 / G) d: the same, finite.  Two groups of random
                +-[0.5, 1) 2^127: sums of both signs overflow early and meet as inf - inf: NaN
  impulses      G groups, group p is 1.0 at position p and +0.0 elsewhere: the answer is a column of the signed Hadamard matrix, taken by sign alone
"""
import functools

import numpy as np

import oracle as O
import rot_model as R

NAMES = ("zeros", "denormal_in", "denormal_out", "cancel", "overflow", "impulses")
SMALL = NAMES[:-1]                      # everything but the G groups of `impulses`
CANCEL_VALUES = (3.25, 2.0 ** -126, 2.0 ** 100)
GROUPS = {"zeros": 4, "denormal_in": 3, "denormal_out": 3, "cancel": 12, "overflow": 4}   # impulses: G


def ngroups(name, G):
    return G if name == "impulses" else GROUPS[name]


def _zeros(G, d, rng, bf16):
    z = np.zeros((4, G), dtype=np.float32)
    z[1] = -0.0
    z[2, 1::2] = -0.0
    z[3, d < 0] = -0.0
    return z


def _denormal_in(G, d, rng, bf16):
    if bf16:
        x = rng.integers(1, 128, (3, G)).astype(np.float64) * 2.0 ** -133 * rng.choice([-1.0, 1.0], (3, G))
        return x.astype(np.float32)
    x = (rng.standard_normal((3, G)) * 1e-41).astype(np.float32)
    x[x == 0] = np.float32(1.4e-45)
    return x


def _denormal_out(G, d, rng, bf16):
    m = 1.0 + rng.integers(0, 128, (3, G)) / 128.0 if bf16 else rng.uniform(1.0, 2.0, (3, G))
    return (m * 2.0 ** -124 * rng.choice([-1.0, 1.0], (3, G))).astype(np.float32)


def _cancel(G, d, rng, bf16):
    rows = []
    for v in CANCEL_VALUES:
        alt = np.where(np.arange(G) % 2 == 0, v, -v)
        rows += [np.full(G, v), alt, v * d.astype(np.float64), v * rng.choice([-1.0, 1.0], G)]
    return np.array(rows, dtype=np.float32)


def _overflow(G, d, rng, bf16):
    near = 0.98828125 if bf16 else 0.99                                  # bfloat16: 253 / 256
    m = 0.5 + rng.integers(0, 128, (2, G)) / 256.0 if bf16 else rng.uniform(0.5, 1.0, (2, G))
    rand = m * 2.0 ** 127 * rng.choice([-1.0, 1.0], (2, G))
    return np.array([2.5 * 2.0 ** 127 / G * d, near * 2.0 ** 127 / G * d, rand[0], rand[1]], dtype=np.float32)


def _impulses(G, d, rng, bf16):
    return np.eye(G, dtype=np.float32)


_MAKERS = {"zeros": _zeros, "denormal_in": _denormal_in, "denormal_out": _denormal_out, "cancel": _cancel, "overflow": _overflow,
           "impulses": _impulses}


@functools.lru_cache(maxsize=None)
def case(name, G, seed, dt=O.F32):
    """one named tensor of type dt (read-only): ngroups(name, G) whole groups and a tail of G - 1 elements"""
    d = R.signs(G, seed)
    rng = np.random.default_rng([NAMES.index(name), G, dt])
    groups = _MAKERS[name](G, d, rng, dt == O.BF16)
    assert groups.dtype == np.float32 and groups.shape == (ngroups(name, G), G)
    xf = np.concatenate([groups.reshape(-1), groups[0, : G - 1]])
    if dt == O.BF16:
        x = O.f32_to_bf16(xf)
        assert np.array_equal(O.bf16_to_f32(x).view(np.uint32), xf.view(np.uint32)), f"{name}: a value is not a bfloat16"
    else:
        x = xf
    x.setflags(write=False)
    return x


def impulse_block(G, dt, first, count):
    """groups first .. first + count - 1 of `impulses` and the tail of G - 1 elements, as a tensor of its own: a tensor that starts on a group
    boundary rotates as the same groups do inside a longer one, so the G groups can be run a block at a time"""
    assert 0 <= first and first + count <= G
    xf = np.zeros(count * G + G - 1, dtype=np.float32)
    xf[np.arange(count) * G + first + np.arange(count)] = 1.0
    xf[count * G] = 1.0                                                      # the tail: the front of group 0
    return xf if dt == O.F32 else O.f32_to_bf16(xf)


def impulse_blocks(G, elems=1 << 19):
    """[(first, count)]: the G groups of `impulses` in blocks of at most `elems` elements"""
    count = max(1, min(G, elems // G))
    return [(first, count) for first in range(0, G, count)]


def cases(G, seed, dt=O.F32, names=NAMES):
    return {name: case(name, G, seed, dt) for name in names}


def is_denormal(xf32):
    """float32 -> bool: nonzero and below 2^-126 in magnitude"""
    a = np.abs(np.asarray(xf32, dtype=np.float32))
    return (a > 0) & (a < np.float32(2.0 ** -126))


def is_neg_zero(xf32):
    return np.asarray(xf32, dtype=np.float32).view(np.uint32) == np.uint32(0x80000000)
