"""crop_cubemap / cubemap_to_panorama / panorama_to_cubemap on the GPU (include/pf_hip.h pf_cube_crop, pf_cube_to_pano) against
the fp64 reference of tests/test_cubemap_ref.py: the float32 image held to the float32 floor of the same formulas, uint8 within one LSB, the seams
(faces back exactly, the means on edges and corners, no jump across an edge or a corner), supersampling against the block mean, the closures with
the panorama tools, batching and determinism, the scalar store path, non-finite parameters, and the fields."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_cubemap_ref import (CORNERS, CUBE_SIZES, EDGES, PANO_OUTPUTS, VIEW_CAMERAS, VIEW_OUTPUTS, block_mean, corner_direction, crop_cube, cube_to_pano,
                                    direction_cube, edge_direction, face_camera, image_bound, look_at, padded_faces, pano_case, pano_to_cube, random_cube,
                                    smooth_panorama, u8_cube, view_case, view_rad)
from tests.test_pano_crop_ref import crop_image
from tests.test_pano_rotate_ref import ROTATIONS, rot_rad, rotate_image

pytestmark = pytest.mark.gpu
PANO_CASES = [(rot, inverse) for rot in ROTATIONS for inverse in (False, True)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(None)
def cube_of(kind, N):
    """(the cube, its padded fp64 faces); read only"""
    cube = {"dir": direction_cube, "pos": lambda n: direction_cube(n) + np.float32(2.0), "u8": u8_cube, "rand": random_cube}[kind](N)
    return cube, padded_faces(cube)


def run_panoramas(kind, out, samples=1):
    """every cube size x rotation x direction at one output size, one call per direction: {(N, rot, inverse): image as numpy}"""
    from perspectivefields_amd import cubemap_to_panorama

    cubes = [gpu(cube_of(kind, N)[0]) for N in CUBE_SIZES]
    got = {}
    for inverse in (False, True):
        jobs = [(n, rot) for n in range(len(CUBE_SIZES)) for rot in ROTATIONS]
        r = np.array([rot for _, rot in jobs])
        img = cubemap_to_panorama(cubes, height=out[0], width=out[1], roll=r[:, 0], pitch=r[:, 1], yaw=r[:, 2], inverse=inverse, cube_index=[n for n, _ in jobs],
                                  samples=samples).cpu().numpy()
        for i, (n, rot) in enumerate(jobs):
            got[CUBE_SIZES[n], rot, inverse] = img[i]
    return got


def run_views(kind, out, samples=1):
    """every cube size x view camera at one output size in one call: {(N, cam): image as numpy}"""
    from perspectivefields_amd import crop_cubemap

    cubes = [gpu(cube_of(kind, N)[0]) for N in CUBE_SIZES]
    jobs = [(n, cam) for n in range(len(CUBE_SIZES)) for cam in VIEW_CAMERAS]
    c = np.array([cam for _, cam in jobs])
    img, _, _ = crop_cubemap(cubes, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=out[0], width=out[1], cube_index=[n for n, _ in jobs],
                             fields=False, samples=samples)
    img = img.cpu().numpy()
    return {(CUBE_SIZES[n], cam): img[i] for i, (n, cam) in enumerate(jobs)}


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("out", PANO_OUTPUTS)
def test_float32_panoramas_match_the_fp64_reference(out):
    """a cube whose texel is its unit direction (value range 2): every kept pixel within 2 x (float32 coordinate floor x local texel step over the
    4 x 4 window of the unfolded face) + 1e-6 of the fp64 image"""
    got = run_panoramas("dir", out)
    worst = 0.0
    for N in CUBE_SIZES:
        cube, P = cube_of("dir", N)
        for rot, inverse in PANO_CASES:
            kept, floor, (k, u, v) = pano_case(rot, inverse, out, N)
            ref = cube_to_pano(cube, rot_rad(*rot), inverse, *out, P=P)
            err = np.abs(got[N, rot, inverse].astype(np.float64) - ref).max(-1)
            bound = image_bound(P, floor, k, u, v)
            worst = max(worst, (err / bound)[kept].max())
            print(f"N {N}, {out}, {rot}, inverse {inverse}: error {err[kept].max():.3e} (error / allowed {(err / bound)[kept].max():.3f}), floor {floor:.3e} texel, "
                  f"{int((~kept).sum())} pixels left out")
            assert (err <= bound)[kept].all(), (N, rot, inverse, (err / bound)[kept].max())
    print(f"{out}: worst error / allowed {worst:.3f}")


@pytest.mark.parametrize("out", VIEW_OUTPUTS)
def test_float32_views_match_the_fp64_reference(out):
    got = run_views("dir", out)
    worst = 0.0
    for N in CUBE_SIZES:
        cube, P = cube_of("dir", N)
        for cam in VIEW_CAMERAS:
            kept, floor, (k, u, v) = view_case(cam, out, N)
            ref = crop_cube(cube, view_rad(cam), *out, P=P)
            err = np.abs(got[N, cam].astype(np.float64) - ref).max(-1)
            bound = image_bound(P, floor, k, u, v)
            if kept.any():
                worst = max(worst, (err / bound)[kept].max())
            print(f"N {N}, {out}, {cam}: error {err[kept].max() if kept.any() else 0.0:.3e}, floor {floor:.3e} texel, {int((~kept).sum())} pixels left out")
            assert (err <= bound)[kept].all(), (N, cam, (err / bound)[kept].max())
    print(f"{out}: worst error / allowed {worst:.3f}")


@pytest.mark.parametrize("out", PANO_OUTPUTS[:2] + VIEW_OUTPUTS[:2])
def test_uint8_within_one_lsb(out):
    """every kept pixel within 1 LSB of the rounded fp64 value"""
    views = out in VIEW_OUTPUTS
    got = run_views("u8", out) if views else run_panoramas("u8", out)
    for N in CUBE_SIZES:
        cube, P = cube_of("u8", N)
        for case in (VIEW_CAMERAS if views else PANO_CASES):
            if views:
                kept, _, _ = view_case(case, out, N)
                ref, img = crop_cube(cube, view_rad(case), *out, P=P), got[N, case]
            else:
                kept, _, _ = pano_case(*case, out, N)
                ref, img = cube_to_pano(cube, rot_rad(*case[0]), case[1], *out, P=P), got[(N, *case)]
            assert img.dtype == np.uint8
            d = np.abs(img.astype(np.float64) - np.clip(np.floor(ref + 0.5), 0, 255)).max(-1)
            assert d[kept].max() <= 1.0, (N, case, d[kept].max())


# ---------------------------------------------------------------- seams: nothing is left out
def test_the_six_face_cameras_return_the_uint8_faces_exactly():
    from perspectivefields_amd import crop_cubemap, cubemap_face_cameras

    cams = cubemap_face_cameras()
    for N in CUBE_SIZES:
        cube = gpu(np.random.default_rng(N).integers(0, 256, (6, N, N, 3), dtype=np.uint8))
        img, up, lat = crop_cubemap(cube, cams["roll"], cams["pitch"], cams["rel_focal"], yaw=cams["yaw"], height=N, width=N)
        assert torch.equal(img, cube), N
        assert up.shape == (6, 2, N, N) and lat.shape == (6, N, N)


@pytest.mark.parametrize("N", [5, 8, 1])
def test_constant_faces_give_the_means_along_edges_and_corners(N):
    from perspectivefields_amd import crop_cubemap

    cube = gpu(np.arange(6, dtype=np.float32)[:, None, None, None] + np.zeros((6, N, N, 3), np.float32))
    looks = [look_at(edge_direction(*e)) for e in EDGES] + [look_at(corner_direction(*c)) for c in CORNERS]
    want = [sum(e) / 2 for e in EDGES] + [sum(c) / 3 for c in CORNERS]
    img, _, _ = crop_cubemap(cube, 0.0, [p for p, _ in looks], 0.5, yaw=[y for _, y in looks], height=1, width=1, fields=False)
    got = img.cpu().numpy().reshape(20, 3)
    print(np.abs(got - np.array(want)[:, None]).max())
    assert np.abs(got - np.array(want)[:, None]).max() <= 1e-5


def test_no_jump_across_an_edge_or_a_corner():
    """a 64 x 64 view of 2 degrees centred on an edge and on a corner of a random N = 8 cube: adjacent output pixels differ by no more than the fp64
    reference's own largest adjacent difference plus 1e-4 of the value range (1); a clamped sampler jumps by a whole texel step here"""
    from perspectivefields_amd import crop_cubemap

    cube, P = cube_of("rand", 8)
    f = 0.5 / np.tan(np.radians(1.0))
    for target in [edge_direction(*e) for e in EDGES] + [corner_direction(*c) for c in CORNERS]:
        p, y = look_at(target)
        img, _, _ = crop_cubemap(gpu(cube), 0.0, p, f, yaw=y, height=64, width=64, fields=False)
        img = img[0].cpu().numpy().astype(np.float64)
        ref = crop_cube(cube, (0.0, np.radians(p), np.radians(y), f, 0.0, 0.0, 0.0), 64, 64, P=P)
        for axis in (0, 1):
            d_gpu, d_ref = np.abs(np.diff(img, axis=axis)).max(), np.abs(np.diff(ref, axis=axis)).max()
            assert d_gpu <= d_ref + 1e-4, (target, axis, d_gpu, d_ref)
        assert np.abs(img - ref).max() <= 1e-4


# ---------------------------------------------------------------- supersampling
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("kind", ["pos", "u8"])
def test_supersampling_is_the_block_mean_of_the_fine_call(kind, S):
    """samples=S equals the S x S block mean of the same call at S times the size with samples=1, for views over the sub-pixels with a ray (the
    cubes hold no 0, so a fine pixel without a ray is the one that is 0): float32 to 1e-5 of the value range, uint8 within 1 LSB.
    The float32 cube is the cube of directions plus 2 (values in [1, 3], range 2).  The two calls evaluate the same points with different float32
    roundings, so they differ by the float32 coordinate floor times the local texel step: up to 1.2e-5 texel at N = 16
    (test_cubemap_ref.test_fp32_floor_and_left_out_pixels_of_the_view_cases) times 0.125 here, an eighth of the tolerance.  A cube of random texels
    (step up to the whole range) turns the same floor into 1.2e-5 of the range, above the tolerance before any mean is taken: measured on an MI355X,
    2.1e-5 at N = 16, S = 3 on the camera with xi = 1.2.  That is the data's step, not the mean's order, so the smooth cube is the input"""
    tol = 1e-5 * 2.0 if kind == "pos" else 1.0
    for out, run in ((PANO_OUTPUTS[1], run_panoramas), (VIEW_OUTPUTS[1], run_views)):
        fine, coarse = run(kind, (S * out[0], S * out[1])), run(kind, out, samples=S)
        for key, img in coarse.items():
            f = fine[key].astype(np.float64)
            valid = f.max(-1) > 0 if run is run_views else np.ones(f.shape[:2], bool)
            d = np.abs(img.astype(np.float64) - block_mean(f, valid, S)).max()
            assert d <= tol, (key, S, d)


# ---------------------------------------------------------------- closures and faces
def test_panorama_to_cubemap_faces_are_the_bits_of_six_crops():
    from perspectivefields_amd import crop_panorama, panorama_to_cubemap

    for dtype in (torch.uint8, torch.float32):
        panos = [gpu(np.random.default_rng(s).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dtype) for s, (h, w) in enumerate([(32, 64), (40, 80)])]
        for samples in (1, 2):
            cube = panorama_to_cubemap(panos, 9, samples=samples)
            assert cube.shape == (2, 6, 9, 9, 3) and cube.dtype == dtype
            for b, pano in enumerate(panos):
                for k in range(6):
                    th = face_camera(k)
                    face, _, _ = crop_panorama(pano, 0.0, np.degrees(th[1]), 0.5, yaw=np.degrees(th[2]), height=9, width=9, fields=False, samples=samples)
                    assert torch.equal(_bits(face[0]), _bits(cube[b, k])), (dtype, samples, b, k)
        assert torch.equal(_bits(panorama_to_cubemap(panos[0], 9)[0]), _bits(panorama_to_cubemap(panos, 9)[0]))


def test_closure_panorama_to_cube_to_panorama():
    """on a smooth panorama (value range 2): no worse than the same chain in fp64 plus 2e-5 of the value range"""
    from perspectivefields_amd import cubemap_to_panorama, panorama_to_cubemap

    src = smooth_panorama(32, 64)
    for N in (16, 8):
        cube = panorama_to_cubemap(gpu(src), N)[0]
        back = cubemap_to_panorama(cube, height=32, width=64)[0].cpu().numpy().astype(np.float64)
        ref = cube_to_pano(pano_to_cube(src.astype(np.float64), N), (0.0, 0.0, 0.0), False, 32, 64)
        e_gpu, e_ref = np.abs(back - src).max(), np.abs(ref - src).max()
        print(f"closure panorama -> cube ({N}) -> panorama: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
        assert e_gpu <= e_ref + 2e-5 * 2.0
    rot = (10.0, 20.0, 30.0)   # the rig turned inside the panorama, then levelled again on the way back
    turned = panorama_to_cubemap(gpu(src), 16, roll=rot[0], pitch=rot[1], yaw=rot[2])[0]
    back = cubemap_to_panorama(turned, height=32, width=64, roll=rot[0], pitch=rot[1], yaw=rot[2], inverse=True)[0].cpu().numpy().astype(np.float64)
    ref = cube_to_pano(pano_to_cube(rotate_image(src.astype(np.float64), rot_rad(*rot), False, 32, 64), 16), rot_rad(*rot), True, 32, 64)
    e_gpu, e_ref = np.abs(back - src).max(), np.abs(ref - src).max()
    print(f"closure turned panorama -> cube -> levelled panorama: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
    assert e_ref <= 0.1 and e_gpu <= e_ref + 2e-5 * 2.0   # a turn in the wrong direction is off by about 1


def test_closure_cube_to_panorama_to_view_against_the_view_of_the_cube():
    from perspectivefields_amd import crop_cubemap, crop_panorama, cubemap_to_panorama

    N = 16
    cube = pano_to_cube(smooth_panorama(64, 128).astype(np.float64), N).astype(np.float32)
    P = padded_faces(cube)
    pano = cubemap_to_panorama(gpu(cube), height=64, width=128)[0]
    pano64 = cube_to_pano(cube, (0.0, 0.0, 0.0), False, 64, 128, P=P)
    for cam in VIEW_CAMERAS[:8]:
        a, _, _ = crop_panorama(pano, cam[0], cam[1], cam[3], cam[4], cam[5], yaw=cam[2], xi=cam[6], height=31, width=47, fields=False)
        b, _, _ = crop_cubemap(gpu(cube), cam[0], cam[1], cam[3], cam[4], cam[5], yaw=cam[2], xi=cam[6], height=31, width=47, fields=False)
        e_gpu = float((a - b).abs().max())
        e_ref = np.abs(crop_image(pano64, view_rad(cam), 31, 47) - crop_cube(cube, view_rad(cam), 31, 47, P=P)).max()
        print(f"closure cube -> panorama -> view against cube -> view, {cam}: GPU difference {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
        assert e_gpu <= e_ref + 2e-5 * 2.0


# ---------------------------------------------------------------- batching, determinism, stores
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_batching_and_determinism(dtype):
    """33 outputs over two cubes of different N (two launches): the same bits alone, permuted and repeated"""
    from perspectivefields_amd import crop_cubemap, cubemap_to_panorama

    rng = np.random.default_rng(8)
    cubes = [gpu(rng.integers(0, 256, (6, N, N, 3), dtype=np.uint8)).to(dtype) for N in (5, 16)]
    n = 33
    rots = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-360, 360, n)], 1)
    foc, xi = rng.uniform(0.3, 1.2, n), np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.0, 1.2, n))
    index = [int(i) for i in rng.integers(0, 2, n)]
    pano = lambda o: cubemap_to_panorama(cubes, height=37, width=75, roll=rots[o, 0], pitch=rots[o, 1], yaw=rots[o, 2], inverse=True, cube_index=[index[i] for i in o], samples=2)
    view = lambda o: crop_cubemap(cubes, rots[o, 0], rots[o, 1], foc[o], yaw=rots[o, 2], xi=xi[o], height=31, width=47, cube_index=[index[i] for i in o], fields=False)[0]
    for run in (pano, view):
        every = list(range(n))
        first, again = run(every), run(every)
        assert first.shape[0] == n and first.dtype == dtype
        perm = [int(i) for i in rng.permutation(n)]
        assert torch.equal(_bits(first), _bits(again)) and torch.equal(_bits(first[perm]), _bits(run(perm)))
        for i in (0, 5, 31, 32):   # both sides of the launch boundary
            assert torch.equal(_bits(first[i]), _bits(run([i])[0])), i
        assert torch.equal(_bits(first[[3, 4, 32]]), _bits(run([3, 4, 32])))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """the Python functions allocate aligned outputs; storage that is not aligned reaches the entry points only through the C interface: 32 x 64
    into an aligned output (vector stores) against the same call into a buffer shifted by one element, and nothing written around it"""
    from perspectivefields_amd import crop_cubemap, cubemap_to_panorama
    from perspectivefields_amd.engine import _check, load_library

    H, W, N = 32, 64, 8
    cube = gpu(u8_cube(N)).to(dtype)
    rots = np.array(ROTATIONS[:3])
    B, n = len(rots), H * W
    lib = load_library()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (0, 1, (ctypes.c_void_p * 1)(cube.data_ptr()), (ctypes.c_int32 * 2)(N, N), 0 if dtype == torch.uint8 else 1, B, (ctypes.c_int32 * B)(*([0] * B)))
    rot = torch.from_numpy(np.radians(rots)).cuda().float().contiguous()
    cam = torch.cat([rot, torch.tensor([[0.6, 0.0, 0.0, 0.8]] * B, device="cuda")], 1).contiguous()
    want_p = cubemap_to_panorama(cube, height=H, width=W, roll=rots[:, 0], pitch=rots[:, 1], yaw=rots[:, 2], samples=2)
    want_v, _, _ = crop_cubemap(cube, rots[:, 0], rots[:, 1], 0.6, yaw=rots[:, 2], xi=0.8, height=H, width=W, fields=False, samples=2)
    for shift in (0, 1):
        for want, call in ((want_p, lambda p: lib.pf_cube_to_pano(*head, rot.data_ptr(), 0, H, W, p, 2, stream())),
                           (want_v, lambda p: lib.pf_cube_crop(*head, cam.data_ptr(), H, W, p, 2, stream()))):
            buf = torch.zeros(B * n * 3 + 4, dtype=dtype, device="cuda")
            out = buf[shift:shift + B * n * 3]
            assert (out.data_ptr() % (4 if dtype == torch.uint8 else 16) != 0) == bool(shift)
            _check(call(out.data_ptr()), None, "cube gather")
            assert torch.equal(_bits(out.reshape(want.shape)), _bits(want))
            assert (buf[:shift] == 0).all() and (buf[shift + B * n * 3:] == 0).all()


# ---------------------------------------------------------------- non-finite parameters, fields
@pytest.mark.parametrize("bad", [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)])
def test_non_finite_angles_give_0_and_leave_the_rest_alone(bad):
    from perspectivefields_amd import crop_cubemap, cubemap_to_panorama

    rots = np.array(ROTATIONS[:3])
    with_bad = np.insert(rots, 1, bad, axis=0)
    for dtype in (torch.uint8, torch.float32):
        cube = gpu(u8_cube(8)).to(dtype)
        good = cubemap_to_panorama(cube, height=37, width=75, roll=rots[:, 0], pitch=rots[:, 1], yaw=rots[:, 2])
        got = cubemap_to_panorama(cube, height=37, width=75, roll=with_bad[:, 0], pitch=with_bad[:, 1], yaw=with_bad[:, 2])
        assert (got[1] == 0).all() and torch.equal(_bits(good), _bits(got[[0, 2, 3]]))
        good, _, _ = crop_cubemap(cube, rots[:, 0], rots[:, 1], 0.6, yaw=rots[:, 2], height=31, width=47, fields=False)
        got, _, _ = crop_cubemap(cube, with_bad[:, 0], with_bad[:, 1], 0.6, yaw=with_bad[:, 2], height=31, width=47, fields=False)
        assert (got[1] == 0).all() and torch.equal(_bits(good), _bits(got[[0, 2, 3]]))


@pytest.mark.parametrize("column", [3, 4, 5, 6])
def test_non_finite_camera_rows_give_0_and_leave_the_rest_alone(column):
    from perspectivefields_amd import crop_cubemap

    cams = np.array(VIEW_CAMERAS[4:8])
    bad = cams.copy()
    bad[1, column] = np.nan if column % 2 else np.inf
    cube = gpu(random_cube(5))
    run = lambda c: crop_cubemap(cube, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=31, width=47, fields=False, samples=2)[0]
    good, got = run(cams), run(bad)
    assert (got[1] == 0).all() and torch.equal(_bits(good[[0, 2, 3]]), _bits(got[[0, 2, 3]]))


def test_fields_are_those_of_the_parameters():
    from perspectivefields_amd import crop_cubemap, cubemap_to_panorama, fields_from_params, panorama_fields

    cube = gpu(u8_cube(5))
    cams = np.array(VIEW_CAMERAS)
    _, up, lat = crop_cubemap(cube, cams[:, 0], cams[:, 1], cams[:, 3], cams[:, 4], cams[:, 5], yaw=cams[:, 2], xi=cams[:, 6], height=31, width=47)
    for i, c in enumerate(VIEW_CAMERAS):
        u, l = fields_from_params(c[0], c[1], c[3], c[4], c[5], height=31, width=47, xi=torch.tensor(c[6], dtype=torch.float64))
        assert torch.equal(_bits(up[i]), _bits(u)) and torch.equal(_bits(lat[i]), _bits(l)), c
    _, up, lat = crop_cubemap(cube, 10.0, 20.0, 0.7, yaw=30.0, height=31, width=47)   # the number 0 for xi: the pinhole entry point
    u, l = fields_from_params(10.0, 20.0, 0.7, height=31, width=47)
    assert torch.equal(_bits(up[0]), _bits(u)) and torch.equal(_bits(lat[0]), _bits(l))
    rots = np.array(ROTATIONS)
    img, up, lat = cubemap_to_panorama(cube, height=37, width=75, roll=rots[:, 0], pitch=rots[:, 1], yaw=rots[:, 2], fields=True)
    u, l = panorama_fields(rots[:, 0], rots[:, 1], height=37, width=75)
    assert img.shape == (4, 37, 75, 3) and torch.equal(_bits(up), _bits(u)) and torch.equal(_bits(lat), _bits(l))
