"""The kernel cases of the attention tests: at least one on each side of every boundary ``sgp_attention_plan`` decides
on.  The plan decides on one thing that changes the kernel, the channel width a wave's registers are built for
(``form`` 1 / 2 / 4 / 8 tiles of 16 columns: boundaries at d = 16 | 24, 32 | 40, 64 | 72), and on the tile counts
(``qtiles``, ``ktiles``: a second tile at L = 17, a partial last tile at every L that is no multiple of 16).
``tests/test_attention_forms.py`` checks the coverage on the host, ``tests/test_gpu_attention.py`` runs every case.
"""
from typing import NamedTuple


class Case(NamedTuple):
    L: int
    d: int
    heads: int
    n_seq: int
    causal: int
    last: bool          # q_first = L - 1
    layout: str         # 'steps': token stride M = n_seq (time-major rows); 'nodes': a sequence's tokens are contiguous

    @property
    def q_first(self):
        return self.L - 1 if self.last else 0

    @property
    def id(self):
        return f"L{self.L}-d{self.d}-h{self.heads}-q{self.n_seq}-c{self.causal}-{'last' if self.last else 'all'}-{self.layout}"


# the form boundaries, each side, both layouts between them
FORM_CASES = [
    Case(17, 8, 3, 3, 1, False, "steps"),
    Case(33, 16, 1, 3, 0, False, "nodes"),
    Case(17, 24, 3, 1, 1, True, "steps"),
    Case(33, 32, 1, 3, 1, False, "nodes"),
    Case(16, 40, 3, 3, 0, False, "steps"),
    Case(33, 64, 1, 3, 1, False, "nodes"),
    Case(17, 72, 3, 1, 0, True, "nodes"),
    Case(33, 128, 1, 3, 1, False, "steps"),
    Case(64, 32, 1, 1, 1, False, "steps"),         # 4 query tiles: a workgroup whose four waves all have work
]

# the sampled product of the issue's sizes
SIZE_CASES = [
    Case(1, 8, 1, 3, 0, False, "steps"),
    Case(1, 32, 3, 1, 1, False, "nodes"),
    Case(2, 24, 3, 65, 1, False, "steps"),
    Case(2, 128, 1, 3, 0, True, "nodes"),
    Case(15, 32, 3, 3, 1, True, "steps"),
    Case(15, 8, 1, 65, 0, False, "nodes"),
    Case(16, 24, 1, 3, 1, False, "nodes"),
    Case(16, 128, 1, 1, 0, True, "steps"),
    Case(17, 32, 1, 65, 0, False, "steps"),
    Case(33, 24, 3, 3, 0, True, "steps"),
    Case(100, 32, 3, 3, 1, False, "steps"),
    Case(100, 8, 1, 3, 1, True, "nodes"),
    Case(100, 128, 1, 1, 0, False, "nodes"),
    Case(130, 24, 3, 3, 0, False, "nodes"),
    Case(130, 32, 1, 1, 1, True, "steps"),
    Case(207, 32, 1, 3, 0, False, "nodes"),
    Case(207, 8, 3, 1, 1, False, "steps"),
    Case(1040, 32, 3, 1, 0, False, "nodes"),
    Case(1040, 128, 1, 1, 1, True, "nodes"),
]

CASES = FORM_CASES + SIZE_CASES

# (L, d, heads, n_seq, causal, q_first) outside the domain, with a word of the reason
OUTSIDE = [
    ((12, 4, 1, 3, 0, 0), "multiple of 8"),
    ((12, 12, 2, 3, 0, 0), "multiple of 8"),
    ((12, 136, 1, 3, 0, 0), "multiple of 8"),
    ((12, 64, 5, 3, 0, 0), "256"),
    ((12, 8, 0, 3, 0, 0), "256"),
    ((0, 8, 1, 3, 0, 0), "at least 1"),
    ((12, 8, 1, 0, 0, 0), "n_seq"),
    ((12, 8, 1, 3, 2, 0), "causal"),
    ((12, 8, 1, 3, 0, 12), "q_first"),
    ((12, 8, 1, 3, 0, -1), "q_first"),
    ((1040, 8, 1, 1 << 26, 0, 0), "2^31"),
]
