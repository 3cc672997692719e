"""No GPU: the stream-order table (tests/stream_order_cases.py) against the header and the oracle's twin of the ABI.

The twin ignores streams, so nothing here is about ordering.  It proves what the GPU runs (test_gpu_stream_order.py)
rely on: that every prototype with a stream is in the table or excluded by name with a reason, that the header says
"synchronises `stream`" for exactly the entry points the table declares so, and, for the cases the twin can run, that
the references hold, that every decoy is a valid input, and that a run on the decoys differs from the true result in
every output -- so that a misordered run cannot pass by accident.
"""
import numpy as np
import pytest

import pointer_offset_cases as P
import stream_order_cases as S


@pytest.fixture(scope="module")
def cpu():
    return P.cpu_backend()


def _on_the_twin(cpu):
    return [c for c in S.CASES if c.runs_on(cpu.lib) and not getattr(c, "self_reference", False)]


def test_every_stream_prototype_is_in_the_table_or_excluded_by_name():
    protos = S.stream_prototypes()
    assert len(protos) == len(set(protos)) == 78, len(protos)
    covered = {e for c in S.CASES for e in c.entries}
    for name in protos:
        assert (name in covered) != (name in S.EXCLUDED), (name, "in a case" if name in covered else "in no case",
                                                            "excluded" if name in S.EXCLUDED else "not excluded")
    assert set(S.EXCLUDED) <= set(protos) and all(len(reason) > 10 for reason in S.EXCLUDED.values())
    assert len(S.EXCLUDED) <= 10


def test_the_header_says_synchronises_for_exactly_the_declared_entry_points():
    protos = [(name, comment) for name, comment, takes in S.header_prototypes() if takes]
    assert len(protos) == 78
    for name, comment in protos:
        wording = "synchronises" if S.header_says_synchronises(comment) else "asynchronous"
        assert wording == S.declared_class(name), (name, "the header's comment reads as " + wording)
    assert set(S.SYNCHRONISES) <= {name for name, _ in protos} and all(S.SYNCHRONISES.values())


def test_the_default_stream_of_the_table_is_the_null_stream():
    assert P.ON.stream is None


def test_tables_have_no_decoy_and_data_planes_do(oracle):
    for case in S.CASES:
        for a in case.args:
            if a.role in ("scratch", "out"):
                a.resolve(oracle)
                assert a.decoy() is None, (case, a.name)
    fixed = [c for c in S.CASES if not any(callable(a.array) for a in c.args)]
    assert len(fixed) > 100
    for case in fixed:
        decoys = [a for a in case.args if a.decoy() is not None]
        inputs = [a for a in case.args if a.role in ("in", "inout", "work") and isinstance(a.array, np.ndarray)]
        assert bool(decoys) == bool(inputs), case
        for a in decoys:
            d = a.decoy()
            assert d.shape == a.array.shape and d.dtype == a.array.dtype
            if a._decoy is None:                            # the default: the same values in reverse order
                assert np.array_equal(d.reshape(-1)[::-1], a.array.reshape(-1)), (case, a.name)


def test_interlopers_and_sensitivity_cases_exist():
    for name in S.INTERLOPERS + S.SENSITIVITY:
        assert name in S.BY_NAME, name
    assert not any(S.synchronises(S.BY_NAME[n]) for n in S.SENSITIVITY)


def test_plain_run_decoy_is_valid_and_distinguishes(cpu, oracle):
    """every case whose entry points the twin exports (found by symbol lookup: the list follows the twin)"""
    cases = _on_the_twin(cpu)
    assert len(cases) >= 51 and any(c in S.EXTRA for c in cases)
    for case in cases:
        run = S.Run(cpu, case, oracle)
        try:
            run.setup()
            refs = S.references(run, oracle)
            run.load("true")
            assert run.call(None) == 0, (case, cpu.lib.va_last_error())
            assert S.mismatches(case, refs, run.outputs(run.work)) == [], case
            assert run.decoys, case
            S.decoy_distinguishes(run, oracle)          # (the check every case gets on the GPU)
            run.load("decoy")
            assert run.call(None) == 0, (case, "the decoy is not a valid input", cpu.lib.va_last_error())
            differing = {n for n, _ in S.mismatches(case, refs, run.outputs(run.work))}
            assert differing == {a.name for a in case.args if a.role in ("out", "inout")}, (case, sorted(differing))
        finally:
            run.free()
