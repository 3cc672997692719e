"""No GPU: the pointer-offset case table (tests/pointer_offset_cases.py) against the oracle's twin of the C ABI.

The twin has no vector kernels and no gates; running the table against it proves that the references, the sentinel
checks and the offset bookkeeping of the table are right before the product meets them (test_gpu_pointer_offsets.py),
and that the twin itself keeps inside late buffers.  Cases whose entry points the twin does not export are listed by
name below; the list is asserted equal to what `hasattr` finds, so it cannot grow silently.
"""
import numpy as np
import pytest

import pointer_offset_cases as P

# entry points (test hooks included) of the table that oracle/libvideoanalysis_cpu.so does not export
TWIN_LACKS = set("""
    va_bg_set_state va_compose_layers_u8 va_contour_workspace_bytes va_detect_peaks_f32 va_detect_peaks_u8
    va_distance_transform_l2_5 va_farneback_workspace_bytes va_fill_poly va_find_contours
    va_find_contours_workspace_bytes va_gaussian_u8_generic va_gaussian_u8_valu va_guo_hall_thinning_batch
    va_guo_hall_thinning_scratch_bytes va_guo_hall_thinning_u8 va_image_statistics_f32 va_image_statistics_u8
    va_jpeg_decode_u8 va_jpeg_decode_workspace_bytes va_jpeg_encode_u8 va_largest_contour va_largest_region
    va_mask_thinning_u8 va_mean_any va_morph_bits_u8 va_normalize va_optical_flow_farneback va_pipeline_create
    va_pipeline_describe va_pipeline_run va_potential_gradients_ragged va_prepare_u8 va_region_links
    va_region_links_workspace_bytes va_rot90 va_sobel5_f64 va_temporal_ranks_u8 va_test_hook_gaussian_f32
    va_test_hook_labelling va_welford_any
    va_distance_map_i32 va_farthest_points va_geodesic_workspace_bytes va_line_scan_u8 va_skeleton_graph
    va_skeleton_graph_workspace_bytes va_warp_affine_u8 va_draw_u8 va_jpeg_encode_sampled_u8
    va_jpeg_decode_sampled_u8 va_jpeg_decode_sampled_workspace_bytes
""".split())


@pytest.fixture(scope="module")
def cpu():
    return P.cpu_backend()


def test_the_twin_lacks_exactly_the_listed_entry_points(cpu):
    used = {e for c in P.CASES for e in c.entries}
    assert {e for e in used if not hasattr(cpu.lib, e)} == TWIN_LACKS
    assert any(c.runs_on(cpu.lib) for c in P.CASES)


def test_every_case_names_its_gate_and_has_a_control():
    for c in P.CASES:
        assert c.gate and (c.gate.startswith("none") or ".hip" in c.gate), c
        combos = P.offset_combos(c.args)
        assert combos[0] == tuple(0 for _ in c.args) and len(set(combos)) == len(combos), c
        movable = [a for a in c.args if len(a.offsets) > 1]
        assert movable, c
        for i, a in enumerate(c.args):                      # every buffer alone at each of its offsets
            for o in a.offsets[1:]:
                assert tuple(o if j == i else 0 for j in range(len(c.args))) in combos, (c, a.name, o)
        if len(movable) > 1:                                # and all of them late at once, not by one amount only
            late = [k for k in combos if all(k[i] for i, a in enumerate(c.args) if len(a.offsets) > 1)]
            assert late and any(len(set(k) - {0}) > 1 for k in late) or all(len(a.offsets) == 2 for a in movable), c


def test_offsets_keep_the_element_type_aligned():
    for itemsize, offsets in P.OFFSETS.items():
        assert offsets[0] == 0 and all(o % itemsize == 0 for o in offsets)
    assert P.OFFSETS[1] == (0, 1, 4, 8) and P.OFFSETS[2] == (0, 2, 8) and P.OFFSETS[4] == (0, 4, 8) and P.OFFSETS[8] == (0, 8)


@pytest.mark.parametrize("name", [c.name for c in P.CASES if not set(c.entries) & TWIN_LACKS])
def test_case_on_the_twin(cpu, oracle, name):
    case = P.BY_NAME[name]
    assert P.run_case(cpu, case, oracle) == 2 * len(P.offset_combos(case.args))


def test_the_helper_sees_a_write_outside_the_payload(cpu):
    """a byte in front of a late buffer, one behind it, and a changed input are each reported"""
    L = cpu.lib
    buf = P.LateBuffer(cpu, 32, 8)
    try:
        for where, at in (("in front", 3), ("behind", 4 + 32)):
            ptr = buf.arm(4, 0xA5, np.arange(32, dtype=np.uint8))
            assert ptr == buf.base.value + 4
            cpu.check(L.va_memset(buf.base.value + at, 0x11, 1, None))
            with pytest.raises(AssertionError, match=where):
                buf.collect(("probe",))
        buf.arm(4, 0x5A, np.arange(32, dtype=np.uint8))
        assert buf.collect(("probe",)).tolist() == list(range(32))
    finally:
        buf.free()
