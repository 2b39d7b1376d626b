"""The calling convention of the wrapper layer: ``_lib.call``'s marshalling against a fake library, the
error-flag finisher and the conversions of ``ops`` on CPU tensors.  No device, no libanirec.so."""
import ctypes as C

import numpy as np
import pytest
import torch

from anime_recommendations_amd import _lib, ops


class FakeLib:
    """Stands in for the loaded library: every ``anirec_*`` attribute records its arguments and returns ``status``."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def anirec_status_string(self, status):
        return b"fake status %d" % status

    def __getattr__(self, name):
        if not name.startswith("anirec_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.status
        return fn


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "_lib", lib)
    assert _lib.load() is lib
    return lib


def test_call_marshals_tensors_none_and_plain_values_in_order(fake):
    t = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    arr, word = (C.c_int32 * 3)(1, 2, 3), C.c_int32(7)
    ref, stream = C.byref(word), C.c_void_p(1234)
    assert _lib.call("anirec_something", t, None, 5, 0.25, arr, ref, stream) is None
    (name, args), = fake.calls
    assert name == "anirec_something"
    assert args[0] == t.data_ptr() and args[1] is None
    assert args[2] == 5 and type(args[2]) is int and args[3] == 0.25 and type(args[3]) is float
    assert args[4] is arr and args[5] is ref and args[6] is stream
    assert len(args) == 7


def test_call_refuses_a_view_that_is_not_contiguous_before_the_call(fake):
    view = torch.arange(16).reshape(4, 4)[:, ::2]
    with pytest.raises(_lib.AnirecError, match="non-contiguous"):
        _lib.call("anirec_something", 1, view, 2)
    assert fake.calls == []


def test_call_passes_an_empty_tensor_as_its_own_address(fake):
    empty = torch.empty(0, dtype=torch.float32)
    _lib.call("anirec_something", empty)
    assert fake.calls[0][1] == (empty.data_ptr(),)


def test_call_checks_the_status_under_the_name_it_called(fake):
    _lib.call("anirec_fine")
    fake.status = 3
    with pytest.raises(_lib.AnirecError) as e:
        _lib.call("anirec_predict_grid_mfma_act", 1)
    assert "anirec_predict_grid_mfma_act failed" in str(e.value)
    assert "fake status 3" in str(e.value) and "(status 3)" in str(e.value)
    assert [c[0] for c in fake.calls] == ["anirec_fine", "anirec_predict_grid_mfma_act"]


# ---------------------------------------------------------------- the error flag
class Unreadable:
    def item(self):
        raise AssertionError("check=False must not read the flag")


def _flag(v):
    return torch.tensor([v], dtype=torch.int32)


def test_err_flag_is_one_int32_word_and_zero_where_it_is_handed_on(monkeypatch):
    f = ops._err_flag("cpu")
    assert f.dtype == torch.int32 and tuple(f.shape) == (1,)
    # an op that reads the flag itself takes what ``torch.empty`` hands out (the dirty-memory tests patch and count it);
    # a flag that may leave the op unread, or meet no clearing in the library, reads 0 whatever that is
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: torch.full(a, 0x7F7F7F7F, **kw))
    assert ops._err_flag("cpu").tolist() == [0x7F7F7F7F]
    f = ops._err_flag("cpu", handed_on=True)
    assert f.dtype == torch.int32 and f.tolist() == [0]


def test_finish_returns_the_result_unchanged_on_a_clear_flag():
    rows, loss = torch.zeros(3), torch.ones(3)
    assert ops._finish(rows, _flag(0), True, "bad") is rows           # cover_levels' shape: one tensor
    got = ops._finish((rows, loss), _flag(0), True, "bad")            # als_half_sweep's: a tuple
    assert isinstance(got, tuple) and got[0] is rows and got[1] is loss


def test_finish_raises_exactly_the_message_on_a_raised_flag():
    with pytest.raises(ValueError) as e:
        ops._finish((torch.zeros(1),), _flag(1), True, "fold_in: anime index out of range")
    assert str(e.value) == "fold_in: anime index out of range"


def test_finish_without_check_appends_the_flag_unread():
    rows, loss, flag = torch.zeros(3), torch.ones(3), Unreadable()
    got = ops._finish(rows, flag, False, "bad")
    assert isinstance(got, tuple) and len(got) == 2 and got[0] is rows and got[1] is flag
    got = ops._finish((rows, loss), flag, False, "bad")
    assert isinstance(got, tuple) and len(got) == 3 and got[0] is rows and got[1] is loss and got[2] is flag


# ---------------------------------------------------------------- the conversions
@pytest.mark.parametrize("keep", [np.array([True, False, True, True]), torch.tensor([1, 0, 1, 1], dtype=torch.uint8),
                                  [1, 0, 1, 1]], ids=["bool-array", "uint8-tensor", "list"])
def test_keep_bytes_takes_bools_bytes_and_lists(keep):
    kp = ops._keep_bytes(keep, 4, "cpu")
    assert kp.dtype == torch.uint8 and kp.is_contiguous() and kp.tolist() == [1, 0, 1, 1]
    assert ops._keep_bytes(None, 4, "cpu") is None


def test_keep_bytes_of_another_length_fails_the_way_the_caller_says():
    with pytest.raises(AssertionError):                 # cosine_topk, rows_topk
        ops._keep_bytes([1, 0, 1], 4, "cpu")
    for what in ("cover_greedy", "fuse_rows"):
        with pytest.raises(ValueError) as e:
            ops._keep_bytes([1, 0, 1], 4, "cpu", what)
        assert str(e.value) == "%s: keep holds one byte per item (4, got 3)" % what


def test_bit_words_keep_the_bits_of_every_input_kind():
    words = np.array([[0x80000001, 0x101], [0xFFFFFFFF, 0]], np.uint32)
    want = words.view(np.int32)
    for x in (words, words.view(np.int32), torch.from_numpy(words.view(np.int32).copy()), np.asfortranarray(words)):
        got = ops._bit_words(x, "cpu", (2, 2), "exclude")
        assert got.dtype == torch.int32 and got.is_contiguous()
        np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(ops._bit_words(words, "cpu").numpy(), want)       # no shape asked: none checked


def test_bit_words_of_another_shape_name_the_argument():
    with pytest.raises(ValueError) as e:
        ops._bit_words(np.zeros((3, 2), np.uint32), "cpu", (2, 2), "exclude")
    assert str(e.value) == "exclude: expected shape (2, 2), got (3, 2)"


def test_recs_uses_the_bit_words_of_ops():
    from anime_recommendations_amd import recs
    assert recs._bit_words is ops._bit_words


def _off(*v):
    return torch.tensor(v, dtype=torch.int64)


def test_check_csr_accepts_empty_lists_between_full_ones():
    ops._check_csr(_off(0, 0, 3, 3, 5), 4, 5, "explain_lists", "history entries")
    ops._check_csr(_off(0), 0, 0, "fold_in", "ratings")


@pytest.mark.parametrize("what,noun", [("explain_lists", "history entries"), ("fold_in", "ratings"),
                                       ("als_half_sweep", "entries")])
@pytest.mark.parametrize("off,n_rows", [((1, 1, 3, 3, 5), 4), ((0, 0, 3, 3, 4), 4), ((0, 3, 2, 3, 5), 4),
                                        ((0, 0, 3, 5), 4), ((0, 0, 3, 3, 5, 5), 4), ((), 0)],
                         ids=["first-1", "last-4", "decreasing", "short", "long", "empty"])
def test_check_csr_refuses_with_the_callers_noun(off, n_rows, what, noun):
    with pytest.raises(ValueError) as e:
        ops._check_csr(_off(*off), n_rows, 5, what, noun)
    assert str(e.value) == "%s: offsets must rise from 0 to the number of %s" % (what, noun)


def test_outputs_have_the_shapes_and_dtypes_asked():
    a, b = ops._outputs("cpu", (torch.int32, 3, 2), (torch.float64, 5))
    assert (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)) == (torch.int32, (3, 2), torch.float64, (5,))
    idx, pos, score, pen = ops._rerank_outputs("cpu", 4, 3)
    assert [t.dtype for t in (idx, pos, score, pen)] == [torch.int32, torch.int32, torch.float32, torch.float32]
    assert all(tuple(t.shape) == (4, 3) for t in (idx, pos, score, pen))
