"""Host side of the counter-based dropout (csrc/dropout.hip): the (threshold, scale) rule and the
four-word device key {seed_lo, seed_hi, step, rank} every launch of a model reads.

Nothing here draws a random number: the keep-bit of an element is a pure function of (seed, rank, step, site,
element index), so the only per-step state is the step word, which the training step writes before its forward
(pipeline.train_step / GraphedTrainStep) from the optimizer's step count."""
import collections
import struct

import torch

MAX_THRESHOLD = 58982       # round(0.9 * 65536)
# attention-probability dropout (csrc/dropout_philox.h QARIG_ATTN_DROPOUT_SITES / _MAX_SK; tests/test_attn_dropout_host.py
# compares them with the header): the site is eight bits of the second counter word, the key index >> 3 the 23 below
ATTN_DROPOUT_SITES = 256
ATTN_DROPOUT_MAX_KEYS = 1 << 26


def threshold_and_scale(p):
    """(T, s) of drop probability p: T = round(p 65536), the true drop rate being T / 65536, and
    s = 65536 / (65536 - T) evaluated in double and rounded to fp32 once (returned as the Python float of that
    fp32 value).  ValueError unless 0 < T <= 58982 (p <= 0.9); NaN is refused."""
    p = float(p)
    if not 0.0 < p < 1.0:        # (NaN fails both comparisons)
        raise ValueError(f"dropout probability must lie in (0, 0.9], got {p}")
    t = int(round(p * 65536.0))
    if not 0 < t <= MAX_THRESHOLD:
        raise ValueError(f"dropout probability must lie in (0, 0.9] and be at least 1/131072, got {p}")
    return t, struct.unpack("f", struct.pack("f", 65536.0 / (65536.0 - t)))[0]


class TokenNoise(collections.namedtuple("TokenNoise", "p_input key p_cond neighbour_range t_input t_cond")):
    """The token-noise state of a model or a scorer (the key second, like the dropout states):
    replace probabilities of the decoder's hr tokens (p_input) and the encoder's lr tokens (p_cond), their
    thresholds (0 = that stream is off) and the neighbour range (0 = the whole codebook)."""
    __slots__ = ()

    @classmethod
    def probabilities(cls, p_input, p_cond, neighbour_range=0):
        """The state without a key yet.  Each probability is 0 or one threshold_and_scale accepts (the scale is
        unused); ValueError otherwise, and for a negative or non-integer range."""
        p_input, p_cond = float(p_input), float(p_cond)
        if isinstance(neighbour_range, bool) or int(neighbour_range) != neighbour_range or neighbour_range < 0:
            raise ValueError(f"token noise: the neighbour range must be an integer >= 0, got {neighbour_range}")
        t_input = threshold_and_scale(p_input)[0] if p_input != 0.0 else 0
        t_cond = threshold_and_scale(p_cond)[0] if p_cond != 0.0 else 0
        return cls(p_input, None, p_cond, int(neighbour_range), t_input, t_cond)

    def with_key(self, key):
        return self._replace(key=key)

    def input_args(self):
        """ops.assemble_tokens(noise=...) of the decoder's hr tokens, or None while p_input is 0."""
        return (self.t_input, self.neighbour_range, self.key.buffer) if self.t_input else None

    def corrupt_cond(self, lr_idx, k_lr):
        """The encoder's lr tokens: one ops.token_noise launch (stream 1), or lr_idx itself while p_cond is 0."""
        if not self.t_cond:
            return lr_idx
        from . import ops
        return ops.token_noise(lr_idx, k_lr, self.t_cond, self.neighbour_range, 1, self.key.buffer)


def _i32(word):
    """A 32-bit word as the int32 value with the same bits."""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word


class DropoutKey:
    """The device key of one model replica: int32[4] {seed_lo, seed_hi, step, rank} (the kernel reads the bits
    as uint32).  set_step writes the step word through a pinned ring (pipeline.PinnedFeed): a non-blocking
    copy on the current stream, the host never waits, and the launches behind it on that stream -- eager
    or replayed from a graph -- read the new step."""

    def __init__(self, seed, rank, device):
        seed, rank = int(seed), int(rank)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"dropout seed must fit 64 bits unsigned, got {seed}")
        if not 0 <= rank < 1 << 32:
            raise ValueError(f"dropout rank must fit 32 bits unsigned, got {rank}")
        self.seed, self.rank, self.step = seed, rank, 0
        self._host = torch.tensor([_i32(seed), _i32(seed >> 32), 0, _i32(rank)], dtype=torch.int32)
        self.buffer = self._host.to(device)
        from .pipeline import PinnedFeed
        self._feed = PinnedFeed(self.buffer)

    def set_step(self, step):
        step = int(step)
        if not 0 <= step < 1 << 32:
            raise ValueError(f"dropout step must fit 32 bits unsigned, got {step}")
        self.step = step
        self._host[2] = _i32(step)
        self._feed.push(self._host)

    @staticmethod
    def threshold_and_scale(p):
        return threshold_and_scale(p)
