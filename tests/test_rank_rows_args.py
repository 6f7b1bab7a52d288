"""daisy_rank_rows_f32 (csrc/rank_rows.hip) checks every argument before its first HIP call: these need no
GPU (the pointers are dummies nobody reads)."""
import ctypes


def _call(N, **over):
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    a = dict(scores=d, m=2, item_num=40, pitch=40, row_users=None, indptr=None, items=None, topk=10, ids=d, sc=None)
    a.update(over)
    return N.lib.daisy_rank_rows_f32(a["scores"], a["m"], a["item_num"], a["pitch"], a["row_users"], a["indptr"], a["items"],
                                     a["topk"], a["ids"], a["sc"], None)


def test_bad_arguments_are_refused_without_a_gpu():
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(64)
    d = ctypes.addressof(buf)
    cases = [(dict(scores=None), "NULL argument"),
             (dict(ids=None), "NULL argument"),
             (dict(pitch=39), "pitch=39 below item_num=40"),
             (dict(topk=0), "topk=0 outside [1, item_num=40]"),
             (dict(topk=129, item_num=400, pitch=400), "topk=129 above the cap of 128"),
             (dict(topk=41), "topk=41 outside [1, item_num=40]"),
             (dict(item_num=0, pitch=0), "item_num=0 outside"),
             (dict(m=-1), "bad row count"),
             (dict(indptr=d, items=d), "an exclusion needs row_users"),
             (dict(row_users=d, indptr=d), "given together or not at all"),
             (dict(row_users=d, items=d), "given together or not at all")]
    for over, text in cases:
        rc = _call(N, **over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        assert N.last_error().startswith("rank_rows_f32:") and text in N.last_error(), (over, N.last_error())
    # no rows: nothing to launch, nothing to check the data pointers for
    assert _call(N, m=0, scores=None, ids=None) == N.DAISY_OK
    # the cap also holds when item_num would allow the cutoff
    assert _call(N, topk=128, item_num=100, pitch=100) == N.DAISY_ERR_ARG and "outside [1, item_num=100]" in N.last_error()


def test_the_python_wrapper_names_the_cap():
    import pytest
    import torch
    from daisyrec_amd import ops
    with pytest.raises(ValueError, match="cap of 128"):
        ops.rank_rows_f32(torch.zeros(2, 300), 129)
    with pytest.raises(TypeError):
        ops.rank_rows_f32(torch.zeros(300), 5)
