"""GPU: every dense op with its device buffers entered at unaligned offsets ("Pointer offsets").

hipMalloc returns 256-byte aligned memory, so a test that uploads into fresh buffers always takes the fast side of a
launcher's pointer gate.  Here every buffer of every case of tests/pointer_offset_cases.py starts 0, 1, 4 or 8 bytes
(as its element type allows) into a sentinel-filled allocation: each buffer late alone, and all of them late at once
by different amounts.  Outputs are compared bit for bit with the reference the family's own test uses, inputs with
what was uploaded, and the bytes around every payload with the sentinel, under two sentinel bytes.  The calls go
through the C ABI; video.ops cannot move a pointer.  No subprocess.
"""
import ctypes as C

import numpy as np
import pytest

import pointer_offset_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return P.hip_backend()


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_case(hip, oracle, name):
    case = P.BY_NAME[name]
    assert P.run_case(hip, case, oracle) == 2 * len(P.offset_combos(case.args))


# ------------------------------------------------------------------ a rejected run leaves the model alone
def _state(L, p, shape):
    state, seen = np.empty(shape, np.float64), C.c_int64()
    assert L.va_bg_get_state(p, state.ctypes.data, state.nbytes, C.byref(seen)) == 0, L.va_last_error()
    return state, seen.value


@pytest.mark.parametrize("late", [1, 2, 3])
def test_rejected_pipeline_run_leaves_the_background_model_unchanged(hip, oracle, late):
    """mfma-i8 pipeline with a running mean: filtered_out_dev off its 4-byte alignment is refused at the top of
    va_pipeline_run, before the model is updated; the next aligned run continues from the untouched state"""
    L = hip.lib
    n, h, w = 2, 32, 64
    clip = P.pipeline_clip(2 * n, h, w, seed=7)
    first = P.chain_reference(oracle, clip[:n], True, 1.0, P.PIPELINE_THRESH[True], True, 4)
    second = P.chain_reference(oracle, clip[n:], True, 1.0, P.PIPELINE_THRESH[True], True, 4, mean=first["state"], n_seen=n)
    p = P.make_pipeline(L, w, h, n, True, 1.0, P.PIPELINE_THRESH[True], True, 4)
    frames, filtered = P.LateBuffer(hip, clip[:n].nbytes, 8), P.LateBuffer(hip, clip[:n].nbytes, 8)
    try:
        assert b"gauss=mfma-i8(" in L.va_pipeline_describe(p)
        for sentinel in P.SENTINELS:
            assert L.va_bg_set_state(p, None, 0, 0) == 0
            assert L.va_pipeline_run(p, frames.arm(0, sentinel, clip[:n]), n, filtered.arm(0, sentinel), None, None, None,
                                     None, None) == 0, L.va_last_error()
            assert filtered.collect("first").tobytes() == first["filtered"].tobytes()
            before, seen = _state(L, p, (h, w))
            assert seen == n and before.tobytes() == first["state"].tobytes()

            rc = L.va_pipeline_run(p, frames.arm(1, sentinel, clip[n:]), n, filtered.arm(late, sentinel), None, None, None,
                                   None, None)
            message = L.va_last_error().decode()
            assert rc == P.VA_ERR_INVALID and "va_pipeline_run" in message and "filtered_out_dev" in message \
                and "aligned" in message, (rc, message)
            assert np.all(filtered.collect("rejected") == sentinel)
            after, seen = _state(L, p, (h, w))
            assert seen == n and after.tobytes() == before.tobytes()

            # frames late by 1 with a model still run: the Gaussian reads the pipeline's own difference image
            assert L.va_pipeline_run(p, frames.arm(1, sentinel, clip[n:]), n, filtered.arm(4, sentinel), None, None, None,
                                     None, None) == 0, L.va_last_error()
            assert filtered.collect("second").tobytes() == second["filtered"].tobytes()
            assert frames.collect("frames").tobytes() == clip[n:].tobytes()
            state, seen = _state(L, p, (h, w))
            assert seen == 2 * n and state.tobytes() == second["state"].tobytes()
    finally:
        L.va_pipeline_destroy(p)
        frames.free()
        filtered.free()


def test_rejected_pipeline_run_without_a_model_names_the_argument(hip):
    """no background model: the single-pass Gaussian reads frames_dev, which must be 16-byte aligned"""
    L = hip.lib
    n, h, w = 2, 32, 64
    clip = P.pipeline_clip(n, h, w)
    for valu, family in ((0, b"mfma-i8"), (1, b"fused-lds")):
        assert L.va_test_hook_gaussian_u8(valu) == 0
        try:
            p = P.make_pipeline(L, w, h, n, False, 1.0, P.PIPELINE_THRESH[False], False, 0)
        finally:
            assert L.va_test_hook_gaussian_u8(0) == 0
        frames, mask = P.LateBuffer(hip, clip.nbytes, 8), P.LateBuffer(hip, clip.nbytes, 8)
        try:
            assert b"gauss=" + family + b"(" in L.va_pipeline_describe(p)
            for late in (1, 4, 8):
                rc = L.va_pipeline_run(p, frames.arm(late, 0xA5, clip), n, None, mask.arm(0, 0xA5), None, None, None, None)
                message = L.va_last_error().decode()
                assert rc == P.VA_ERR_INVALID and "va_pipeline_run" in message and "frames_dev" in message \
                    and "aligned" in message, (family, late, rc, message)
                assert np.all(mask.collect("rejected") == 0xA5)
        finally:
            L.va_pipeline_destroy(p)
            frames.free()
            mask.free()


# ------------------------------------------------------------------------------- the promised rejections
@pytest.mark.parametrize("entry", sorted(P.REJECTIONS))
def test_misaligned_pointer_is_refused_and_nothing_is_enqueued(hip, entry):
    """every pointer the header promises VA_ERR_INVALID for, one at a time, on sentinel-filled buffers: the code, a
    message that names the call and the alignment, and every buffer of the call untouched afterwards (the code and
    the message alone are also checked without a GPU, tests/test_entry_guards_host.py)"""
    L = hip.lib
    names = [a.name for a in P.REJECTIONS[entry] if isinstance(a, P.ptr)]
    bufs = {n: P.LateBuffer(hip, 512, 16) for n in names}
    try:
        for sentinel in P.SENTINELS:
            for name, by in P.rejection_calls(entry):
                address = {n: bufs[n].arm(by if n == name else 0, sentinel) for n in names}
                rc = getattr(L, entry)(*P.rejection_args(entry, address.__getitem__))
                said = L.va_last_error().decode()
                assert rc == P.VA_ERR_INVALID and entry in said and "aligned" in said, (entry, name, by, rc, said)
                for n in names:
                    assert np.all(bufs[n].collect((entry, name, n)) == sentinel), (entry, name, n)
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("late", [{"frames": 4}, {"frames": 8}, {"filtered": 4}, {"filtered": 8}, {"frames": 8, "filtered": 4}])
def test_float32_pipeline_refuses_misaligned_frames(hip, late):
    """float32 pipelines need 16-byte aligned frames_dev and filtered_out_dev (the fused row pass): refused before
    the EMA state is touched"""
    L = hip.lib
    n, h, w, c = 2, 33, 72, 3                   # (rows of whole 16-byte vectors: the fused family)
    clip = np.random.default_rng(5).random((n, h, w, c), dtype=np.float32)
    p = P.make_pipeline(L, w, h, n, P.BG_EMA, 2.0, -1, False, 0, dtype=P.VA_F32, channels=c, bg_rate=0.02)
    frames, filtered = P.LateBuffer(hip, clip.nbytes, 8), P.LateBuffer(hip, clip.nbytes, 8)
    try:
        assert b"gauss=f32-ema-row+col-march(" in L.va_pipeline_describe(p), L.va_pipeline_describe(p)
        state, seen = np.empty((h, w, c), np.float32), C.c_int64()
        for sentinel in P.SENTINELS:
            assert L.va_bg_set_state(p, None, 0, 0) == 0
            assert L.va_pipeline_run(p, frames.arm(0, sentinel, clip), n, filtered.arm(0, sentinel), None, None, None, None,
                                     None) == 0, L.va_last_error()
            assert L.va_bg_get_state(p, state.ctypes.data, state.nbytes, C.byref(seen)) == 0 and seen.value == n
            before = state.tobytes()
            rc = L.va_pipeline_run(p, frames.arm(late.get("frames", 0), sentinel, clip), n,
                                   filtered.arm(late.get("filtered", 0), sentinel), None, None, None, None, None)
            said = L.va_last_error().decode()
            assert rc == P.VA_ERR_INVALID and "va_pipeline_run" in said and "aligned" in said, (late, rc, said)
            assert np.all(filtered.collect("rejected") == sentinel)
            assert frames.collect("frames").tobytes() == clip.tobytes()
            assert L.va_bg_get_state(p, state.ctypes.data, state.nbytes, C.byref(seen)) == 0
            assert seen.value == n and state.tobytes() == before, late
    finally:
        L.va_pipeline_destroy(p)
        frames.free()
        filtered.free()
