"""What the device data builds share (csrc/devprep.h; _lib.workspace): the workspace sizes the eight builds ask for, against
figures recorded from the library BEFORE the carving moved into one place -- a caller that sized a workspace then holds a
valid one now --, and the Python helper's refusal.  Host arithmetic only: no GPU."""
import pytest

from score_amd import _lib

B = 2 ** 31
# (arguments, bytes): the first count at 63, 64, 65 and a large value, then the sizes that are refused
SIZES = {
    "score_point_hist": [((63,), 33792), ((64,), 33792), ((65,), 34816), ((1000003,), 18032640), ((0,), -1), ((B,), -1)],
    "score_graph_build": [((63, 10, 20, 3), 34816), ((64, 20, 10, 3), 34816), ((65, 64, 64, 1), 36352),
                          ((1000003, 5000, 70001, 11), 29114880), ((0, 10, 20, 3), -1), ((B, 10, 20, 3), -1), ((63, 0, 20, 3), -1),
                          ((63, 10, 0, 3), -1), ((63, 10, 20, 0), -1), ((63, 1048576, 1, 2048), -1)],
    "score_target_build": [((63, 100), 35584), ((64, 64), 35584), ((65, 65), 37376), ((1000003, 4097), 34052096), ((0, 100), -1),
                           ((B, 100), -1), ((63, 0), -1)],
    "score_pop_items": [((63,), 1024), ((64,), 1280), ((65,), 1536), ((1000003,), 12002560), ((0,), -1)],
    "score_log_remap": [((63, 1), 36864), ((64, 3), 37376), ((65, 8), 39936), ((1000003, 4), 58036992), ((0, 1), -1), ((B, 1), -1),
                        ((63, 0), -1), ((63, 9), -1)],
    "score_log_compact": [((63,), 1024), ((64,), 1280), ((65,), 1536), ((1000003,), 12002560), ((0,), -1), ((B,), -1)],
    "score_ccmr_prep": [((63, 100), 36096), ((64, 64), 35328), ((65, 4097), 101376), ((1000003, 17770), 18317568), ((0, 50), 2304),
                        ((-1, 50), -1), ((B, 50), -1), ((63, 0), -1)],
    "score_neg_lists": [((63,), 33792), ((64,), 33792), ((65,), 34816), ((1000003,), 18032640), ((0,), 1024), ((-1,), -1),
                        ((B,), -1)],
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_workspace_sizes_are_the_recorded_ones(name):
    fn = getattr(_lib.load(), name + "_temp_bytes")
    assert [(args, fn(*args)) for args, _ in SIZES[name]] == SIZES[name]
    assert sum(1 for _, size in SIZES[name] if size > 0) >= 4 and any(size == -1 for _, size in SIZES[name])


class _StubLib(object):
    def __init__(self, size):
        self.size, self.calls = size, []

    def score_stub_temp_bytes(self, *args):
        self.calls.append(args)
        return self.size


def test_workspace_refuses_a_negative_size_before_it_allocates(monkeypatch):
    import torch
    made = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: made.append(a) or real_empty(*a, **kw))
    stub = _StubLib(-1)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    with pytest.raises(_lib.ScoreHipError, match="score_stub_temp_bytes failed: unsupported shape"):
        _lib.workspace("score_stub", "cpu", 5, 7)
    assert stub.calls == [(5, 7)] and made == []
    stub.size = 96                                 # (and a size it grants is allocated as it is)
    temp, nbytes = _lib.workspace("score_stub", "cpu", 3)
    assert nbytes == 96 and temp.dtype == torch.uint8 and tuple(temp.shape) == (96,) and len(made) == 1
