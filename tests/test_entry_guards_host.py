"""Host: the argument guards of the entry points that sit beside their kernels (labelling, contours, geodesic maps,
Gaussian, pointwise, morphology, stencils).  Every call here is refused with VA_ERR_INVALID before anything touches a
device or a pointer, so no GPU is needed: the pointers are made-up addresses.  Where an entry has several guards the
cases are in the order the entry checks them, and each case trips exactly one more than the one before.  The
misaligned pointers the header promises VA_ERR_INVALID for come from the table of tests/pointer_offset_cases.py, one
pointer at a time (tests/test_gpu_pointer_offsets.py repeats them on real buffers and checks that nothing was
written)."""
import pytest

INVALID = -22
P, Q = 4096, 8192                 # distinct non-NULL addresses; never dereferenced
BIG = (1 << 15, 1 << 14)          # h, w of a frame of 2^29 pixels
TOO_BIG = "frames above 2^29 pixels are not supported"
U8 = 0

CASES = [
    ("va_gauss_taps_q8", (1.0, None, None, 0), "va_gauss_taps_q8: NULL argument"),
    ("va_gauss_taps_f32", (1.0, None, None, 0), "va_gauss_taps_f32: NULL argument"),
    ("va_gaussian_f32", (P, Q, 1) + BIG + (1, 1.0, None), "va_gaussian_f32: " + TOO_BIG),
    ("va_gaussian_f32", (P, P, 1, 4, 4, 1, 1.0, None), "va_gaussian_f32: src/dst must be distinct non-NULL"),
    ("va_gaussian_f32", (P, Q, 1, 4, 0, 1, 1.0, None), "va_gaussian_f32: bad shape (1,4,0,1)"),
    ("va_gaussian_u8_valu", (P, P, 1, 4, 4, 1, 1.0, None), "va_gaussian_u8_valu: bad pointers"),
    ("va_gaussian_u8_valu", (P, Q, 1, 4, 4, 3, 1.0, None), "va_gaussian_u8_valu: bad shape"),
    ("va_gaussian_u8_generic", (P, Q, -1, 4, 4, 1, 1.0, None), "va_gaussian_u8_generic: bad shape"),
    ("va_welford_any", (P, U8, P, None, 0, 1, 16, None), "va_welford_any: NULL argument"),
    ("va_rot90", (P, P, 1, 4, 4, 1, 1, None), "va_rot90: src/dst must be distinct non-NULL"),
    ("va_rot90", (P, Q, 1, 0, 4, 1, 1, None), "va_rot90: bad shape (1,0,4)"),
    ("va_morph_u8", (P, Q, 1) + BIG + (0, 0, 3, None), "va_morph_u8: " + TOO_BIG),
    ("va_morph_u8", (P, P, 1, 4, 4, 0, 0, 3, None), "va_morph_u8: src/dst must be distinct non-NULL"),
    ("va_morph_u8", (P, Q, -1, 4, 4, 0, 0, 3, None), "va_morph_u8: bad shape (-1,4,4)"),
    ("va_morph_u8", (P, Q, 1, 4, 4, 7, 0, 3, None), "va_morph_u8: bad op 7"),
    ("va_morph_bits_u8", (P, Q, 1) + BIG + (0, 0, 3, None), "va_morph_bits_u8: " + TOO_BIG),
    ("va_morph_bits_u8", (P, None, 1, 4, 4, 0, 0, 3, None), "va_morph_bits_u8: NULL argument"),
    ("va_morph_bits_u8", (P, Q, 1, 4, -4, 0, 0, 3, None), "va_morph_bits_u8: bad shape"),
    ("va_label_i32", (P, P, P, 1) + BIG + (4, P, 1 << 40, None), "va_label_i32: " + TOO_BIG),
    ("va_label_i32", (P, P, None, 1, 4, 4, 4, P, 1 << 40, None), "va_label_i32: NULL argument"),
    ("va_label_i32", (P, P, P, 1, 0, 4, 4, P, 1 << 40, None), "va_label_i32: bad shape (1,0,4)"),
    ("va_label_i32", (P, P, P, 1, 4, 4, 4, P, 1, None), "va_label_i32: workspace of 1 bytes < required"),
    ("va_moments_i64", (P, 1, 0, 4, 1, P, None), "va_moments_i64: bad shape (1,0,4)"),
    ("va_moments_i64", (None, 1, 4, 4, 1, P, None), "moments: NULL argument / max_labels <= 0"),
    ("va_moments_i64", (P, 1, 4, 4, 0, P, None), "moments: NULL argument / max_labels <= 0"),
    ("va_largest_region", (P, P, P, -1, 4, 4, 1, P, None, None, None), "va_largest_region: bad shape (-1,4,4)"),
    ("va_largest_region", (P, None, P, 1, 4, 4, 1, P, None, None, None), "largest_region: NULL argument"),
    ("va_test_hook_labelling", (6, 0), "va_test_hook_labelling: bad arguments"),
    ("va_test_hook_labelling", (0, -1), "va_test_hook_labelling: bad arguments"),
    ("va_detect_peaks_u8", (P, Q, 1) + BIG + (0, None), "va_detect_peaks_u8: " + TOO_BIG),
    ("va_detect_peaks_u8", (P, P, 1, 4, 4, 0, None), "va_detect_peaks_u8: bad pointers"),
    ("va_detect_peaks_u8", (P, Q, 1, 4, 0, 0, None), "va_detect_peaks_u8: bad shape"),
    ("va_detect_peaks_f32", (P, Q, 1) + BIG + (0, None), "va_detect_peaks_f32: " + TOO_BIG),
    ("va_detect_peaks_f32", (None, Q, 1, 4, 4, 0, None), "va_detect_peaks_f32: bad pointers"),
    ("va_detect_peaks_f32", (P, Q, -1, 4, 4, 0, None), "va_detect_peaks_f32: bad shape"),
    ("va_image_statistics_u8", (P, Q, None, 1) + BIG + (0, 1, 0.0, 0, None), "va_image_statistics_u8: " + TOO_BIG),
    ("va_image_statistics_u8", (P, None, None, 1, 4, 4, 0, 1, 0.0, 0, None), "va_image_statistics_u8: NULL argument"),
    ("va_image_statistics_u8", (P, Q, None, 1, 4, 4, 0, -1, 0.0, 0, None), "va_image_statistics_u8: bad shape"),
    ("va_image_statistics_u8", (P, Q, None, 1, 4, 4, 2, 1, 0.0, 0, None), "va_image_statistics_u8: kernel must be"),
    ("va_image_statistics_f32", (P, Q, None, 1) + BIG + (0, 1, 0.0, 0, None), "va_image_statistics_f32: " + TOO_BIG),
    ("va_image_statistics_f32", (None, Q, None, 1, 4, 4, 0, 1, 0.0, 0, None), "va_image_statistics_f32: NULL argument"),
    ("va_image_statistics_f32", (P, Q, None, 0, 0, 4, 0, 1, 0.0, 0, None), "va_image_statistics_f32: bad shape"),
    ("va_image_statistics_f32", (P, Q, None, 1, 4, 4, -1, 1, 0.0, 0, None), "va_image_statistics_f32: kernel must be"),
    ("va_mask_thinning_u8", (None, P, Q, 4, 4, None, None), "va_mask_thinning_u8: NULL argument"),
    ("va_mask_thinning_u8", (P, Q, P + Q, 4, 0, None, None), "va_mask_thinning_u8: bad shape"),
    ("va_largest_contour", (P, 1) + BIG + (P, 8, P, None, P, P, 1 << 40, None), "va_largest_contour: " + TOO_BIG),
    ("va_largest_contour", (P, 1, 4, 4, P, 8, P, None, None, P, 1 << 40, None), "va_largest_contour: NULL argument"),
    ("va_largest_contour", (P, 1, 4, 4, P, 0, P, None, P, P, 1 << 40, None), "va_largest_contour: bad shape"),
    ("va_largest_contour", (P, 1, 4, 4, P, 8, P, None, P, P, 1, None), "va_largest_contour: workspace of 1 bytes"),
    ("va_find_contours", (P, 1) + BIG + (P, P, P, P, 1, P, 1, P, 1 << 40, None), "va_find_contours: " + TOO_BIG),
    ("va_find_contours", (P, 1, 4, 4, P, P, P, P, 1, P, 1, None, 1 << 40, None), "va_find_contours: NULL argument"),
    ("va_find_contours", (P, -1, 4, 4, P, P, P, P, 1, P, 1, P, 1 << 40, None), "va_find_contours: bad shape"),
    ("va_find_contours", (P, 1, 4, 4, P, P, P, P, -1, P, 1, P, 1 << 40, None), "va_find_contours: negative capacity"),
    ("va_find_contours", (P, 1, 4, 4, P, P, P, P, 1, P + 4, 1, P, 1 << 40, None), "must be 8-byte aligned"),
    ("va_find_contours", (P, 1, 4, 4, P, P, P, P, 1, P, 1, P, 1, None), "va_find_contours: workspace of 1 bytes"),
]
# the three geodesic entries share their first four guards; the frame of 2^29 pixels is also wider than 8192 columns,
# so it shows that the size is checked first
GEODESIC = {
    "va_distance_map_i32": lambda n, h, w, ws, nb: (P, n, h, w, P, P, 1, None, None, 0, P, ws, nb, None),
    "va_distance_map_path": lambda n, h, w, ws, nb: (P, n, h, w, P, P, 8, P, ws, nb, None),
    "va_farthest_points": lambda n, h, w, ws, nb: (P, n, h, w, None, P, P, P, P, None, 0, None, ws, nb, None),
}
for _name, _args in GEODESIC.items():
    CASES += [
        (_name, _args(1, *BIG, P, 1 << 40), _name + ": " + TOO_BIG),
        (_name, _args(-1, 4, 4, P, 1 << 40), _name + ": bad shape"),
        (_name, _args(1, 4, 8193, P, 1 << 40), _name + ": frames wider than 8192 columns are not supported"),
        (_name, _args(1, 4, 4, None, 1 << 40), _name + ": workspace of"),
        (_name, _args(1, 4, 4, P, 1), _name + ": workspace of 1 bytes < required"),
    ]
CASES += [
    ("va_distance_map_i32", (None, 1, 4, 4, P, P, 1, None, None, 0, P, P, 1 << 40, None), "va_distance_map_i32: NULL argument"),
    ("va_distance_map_i32", (P, 1, 4, 4, P, P, 1, P, None, 0, P, P, 1 << 40, None), "end points without counts"),
    ("va_distance_map_path", (P, 1, 4, 4, P, P, 0, P, P, 1 << 40, None), "va_distance_map_path: NULL argument"),
    ("va_farthest_points", (P, 1, 4, 4, None, None, P, P, P, None, 0, None, P, 1 << 40, None),
     "va_farthest_points: NULL argument"),
    ("va_farthest_points", (P, 1, 4, 4, None, P, P, P, P, P, 0, None, P, 1 << 40, None),
     "va_farthest_points: path without npath / max_points"),
]


@pytest.fixture(scope="module")
def lib():
    from video import _hip
    return _hip.load_library()


def _misaligned():
    """every pointer that include/videoanalysis_hip.h promises VA_ERR_INVALID for when it is misaligned, one at a time
    (the table of tests/pointer_offset_cases.py; on the GPU the same calls run on sentinel-filled buffers)"""
    import pointer_offset_cases as T
    return [(entry, name, by) for entry in sorted(T.REJECTIONS) for name, by in T.rejection_calls(entry)]


@pytest.mark.parametrize("entry,name,by", _misaligned(), ids=["%s-%s" % c[:2] for c in _misaligned()])
def test_misaligned_pointer_is_refused_and_named(lib, entry, name, by):
    import pointer_offset_cases as T
    names = [a.name for a in T.REJECTIONS[entry] if isinstance(a, T.ptr)]
    args = T.rejection_args(entry, lambda n: P * (1 + names.index(n)), name, by)
    rc = getattr(lib, entry)(*args)
    said = lib.va_last_error().decode()
    assert rc == INVALID and entry in said and "aligned" in said, (entry, name, by, rc, said)


def test_every_promised_alignment_is_in_the_table():
    """the calls whose header text names an alignment or a misaligned pointer"""
    import pointer_offset_cases as T
    assert set(T.REJECTIONS) == {
        "va_find_contours", "va_skeleton_graph", "va_region_links", "va_simplify_rdp", "va_simplify_visvalingam",
        "va_curves_equidistant", "va_compose_layers_u8", "va_draw_u8", "va_draw_contours_u8", "va_jpeg_encode_u8",
        "va_jpeg_encode_sampled_u8", "va_jpeg_encode_optimized_u8", "va_jpeg_optimal_tables", "va_jpeg_decode_u8",
        "va_jpeg_decode_sampled_u8", "va_jpeg_decode_split_u8"}
    for entry, args in T.REJECTIONS.items():
        assert len(args) == len(_signature(entry)), entry


def _signature(entry):
    from video import _hip
    return _hip.SIGNATURES[entry][1]


@pytest.mark.parametrize("entry,args,message", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refused_before_anything_is_touched(lib, entry, args, message):
    rc = getattr(lib, entry)(*args)
    said = lib.va_last_error().decode()
    print(entry, rc, said)
    assert rc == INVALID and message in said, (entry, args, rc, said)
