"""Objects pasted into backgrounds on the GPU (include/pf_hip.h pf_composite; perspectivefields_amd.composite_objects, PerspectiveFields.composite)
against the fp64 reference of tests/test_composite_ref.py on its fixed inputs; the exact cases; the block-mean property; the hard edge against
transform_fields; inactive rows; independence of the launch; the chain from placement_search; the other forms of the arguments.

Tolerances (derived in the reference file's docstring, not fitted): per pixel the fp32 source position's error bound times the
largest difference among the object's values around the pixel's taps, and the one rounding of the output.  float32 outputs lie within that bound;
uint8 outputs are within 1 LSB everywhere and equal to the reference's wherever its fp64 value is farther from a rounding tie than the bound; the
dyadic cases and the identity are equal bit for bit, ties included.  With the hard edge the borderline pixels (|A - 1/2| < 1e-3) are left out.  Outside
the box, and wherever nothing is covered, the output is the background's bits: checked on float32 backgrounds with NaN pixels of a given payload."""
import functools

import numpy as np
import pytest
import torch

from tests.test_composite_ref import (BG_HW, CASES, OBJ_HW, OFFSETS, VARIANTS, alpha_plane, case_id, case_inputs, case_reference, is_dyadic, make_place, picture,
                                      ref_composite, tie_distance, variant_size)
from tests.test_placement_search_ref import PLANT_ROTATIONS, PLANT_SCALES, planted_search

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC12345   # a quiet NaN with a payload: a copy keeps it, arithmetic need not


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # a copy: the cached inputs are read-only


def same_bits(a, b):
    a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def with_nan_outside(bg, box):
    """a float32 background with NaN pixels of a known payload at up to three places outside the box"""
    bg = np.array(bg)
    free = np.argwhere(~box)
    for r, c in free[:: max(1, len(free) // 3)][:3]:
        bg[r, c].view(np.uint32)[:] = NAN_BITS
    return bg


def paste(c, bg=None, **over):
    from perspectivefields_amd import composite_objects

    b, obj, al, place = case_inputs(c)
    kw = dict(scale=place[0], rotation=place[1], offset=place[2:4], size=place[4:6], alpha=dev(al), opacity=c["opacity"], edge=c["edge"], samples=c["samples"],
              return_coverage=True)
    kw.update(over)
    return composite_objects(dev(b if bg is None else bg), dev(obj), **kw)


def check(got, cov, ref, bg, edge, what):
    """the device's picture and coverage against ref_composite's dict; returns the largest error as a share of the allowed (value, coverage)"""
    got, cov = got.cpu().numpy(), cov.cpu().numpy()
    assert got.dtype == bg.dtype and got.shape == bg.shape and cov.dtype == np.float32 and cov.shape == bg.shape[:2], what
    sure = ~ref["borderline"] if edge == "hard" else np.ones(cov.shape, dtype=bool)
    # outside the box, and with the hard edge outside the silhouette: the background's bits and no coverage
    keep = sure & (~ref["box"] if edge == "soft" else ref["cov"] == 0)
    assert got[keep].tobytes() == bg[keep].tobytes() and not cov[keep].any(), what
    if edge == "hard":
        assert np.array_equal((cov > 0)[sure], (ref["cov"] > 0)[sure]), what
    # wherever the device covers nothing, it copies
    none = cov == 0
    assert got[none].tobytes() == bg[none].tobytes(), what
    cmp = sure & ref["box"]
    if not cmp.any():
        return 0.0, 0.0
    e_cov = np.abs(cov.astype(np.float64) - ref["cov"])[cmp]
    assert (e_cov <= ref["tol_cov"][cmp]).all(), (what, e_cov.max())
    err = np.abs(got.astype(np.float64) - ref["value"])[cmp]
    tol = ref["tol"][cmp]
    if got.dtype == np.float32:
        assert (err <= tol).all(), (what, err.max(), (err / np.maximum(tol, 1e-300)).max())
        share = float((err / np.maximum(tol, 1e-300)).max())
    else:
        # everywhere, no pixel near a tie left out (the hard edge's borderline pixels are no such pixels: they may change sides as a whole)
        assert np.abs(got.astype(np.int64) - ref["out"].astype(np.int64))[sure].max() <= 1 and (err <= 0.5 + tol).all(), what
        decided = tie_distance(ref["value"][cmp]) > tol
        assert np.array_equal(got[cmp][decided], ref["out"][cmp][decided]), (what, int((got[cmp] != ref["out"][cmp])[decided].sum()))
        share = float(((err - 0.5) / np.maximum(tol, 1e-300)).max())   # how far past its half step the worst value lies, of the allowed
    return share, float((e_cov / np.maximum(ref["tol_cov"][cmp], 1e-300)).max())


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: case_id(CASES[i]))
def test_against_the_reference(i):
    c, ref = CASES[i], case_reference(CASES[i])
    bg = case_inputs(c)[0]
    if c["dtype"] == "float32":
        bg = with_nan_outside(bg, ref["box"])
    got, cov = paste(c, bg)
    share = check(got, cov, ref, bg, c["edge"], case_id(c))
    print(f"{case_id(c)}: largest error / allowed {share[0]:.3f}, coverage {share[1]:.3f}")
    if c["dtype"] == "float32":   # the NaN pixels outside the box came through with their payload
        assert int((got.cpu().numpy().view(np.uint32) == NAN_BITS).sum()) == int((bg.view(np.uint32) == NAN_BITS).sum()) > 0
    if is_dyadic(c):   # every position, weight, sum and the blend is a dyadic rational of few bits: no tolerance, uint8 ties included
        want = np.where(ref["box"][..., None], ref["out"], bg)   # bg carries the NaN pixels outside the box; np.where moves bits
        assert same_bits(got, want) and same_bits(cov, ref["cov"].astype(np.float32)), case_id(c)


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_identity_copies_the_object(dtype):
    from perspectivefields_amd import composite_objects

    bg, obj, al = picture("bg", dtype), picture("obj", dtype), alpha_plane("ellipse")
    for off in OFFSETS:
        ref = ref_composite(bg, obj, al, make_place((1.0, 0.0), off))
        got, cov = composite_objects(dev(bg), dev(obj), offset=off, alpha=dev(al), return_coverage=True)
        assert same_bits(got, ref["out"]) and same_bits(cov, ref["cov"].astype(np.float32)), off
    got = composite_objects(dev(bg), dev(obj), offset=OFFSETS[0])   # opaque, no coverage asked for
    want = np.array(bg)
    want[13:28, 22:34] = obj
    assert same_bits(got, want)


def test_garbage_under_a_zero_alpha_does_not_leak():
    from perspectivefields_amd import composite_objects

    bg, obj, al = picture("bg", "float32"), np.array(picture("obj", "float32")), np.array(alpha_plane("ellipse"))
    kw = dict(scale=1.5, rotation=10.0, offset=(5, 7), opacity=0.5, samples=2)
    clean = composite_objects(dev(bg), dev(obj), alpha=dev(al), **kw)
    obj[al == 0] = np.nan
    al[0, 0] = np.nan
    dirty = composite_objects(dev(bg), dev(obj), alpha=dev(al), **kw)
    assert same_bits(clean, dirty) and torch.isfinite(dirty).all()


@pytest.mark.parametrize("S", (2, 3))
def test_block_mean_property(S):
    """samples = S against the S x S block mean of samples = 1 on the replicated background under scale s S, offset S, size S: to the two calls' bounds"""
    from perspectivefields_amd import composite_objects

    bg, obj, al = picture("bg", "float32"), picture("obj", "float32"), alpha_plane("quarter")
    variant, off = (1.5, 10.0), (13, 22)
    hb, wb = variant_size(variant)
    big_bg = np.repeat(np.repeat(bg, S, axis=0), S, axis=1)
    big_place = (variant[0] * S, variant[1], off[0] * S, off[1] * S, hb * S, wb * S)
    r_small, r_big = ref_composite(bg, obj, al, make_place(variant, off), 0.5, "soft", S), ref_composite(big_bg, obj, al, big_place, 0.5, "soft", 1)
    small = composite_objects(dev(bg), dev(obj), scale=variant[0], rotation=variant[1], offset=off, size=(hb, wb), alpha=dev(al), opacity=0.5, samples=S)
    big = composite_objects(dev(big_bg), dev(obj), scale=big_place[0], rotation=variant[1], offset=big_place[2:4], size=big_place[4:6], alpha=dev(al), opacity=0.5)
    mean = lambda a: a.reshape(BG_HW[0], S, BG_HW[1], S, 3).mean(axis=(1, 3))
    err = np.abs(mean(big.cpu().numpy().astype(np.float64)) - small.cpu().numpy().astype(np.float64))
    allowed = r_small["tol"] + mean(r_big["tol"])
    print(f"S = {S}: largest difference {err.max():.2e}, largest allowed {allowed.max():.2e}")
    assert (err <= allowed).all() and err[~r_small["box"]].max() == 0


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != (1.5, 0.0)])
def test_hard_edge_pastes_the_pixels_the_search_scored(variant):
    from perspectivefields_amd import composite_objects, transform_fields

    bg, obj, al = picture("bg", "float32"), picture("obj", "float32"), alpha_plane("ellipse")
    up = np.stack([np.ones(OBJ_HW, dtype=np.float32), np.zeros(OBJ_HW, dtype=np.float32)])
    lat = np.where(al == 1, np.float32(0), np.float32(np.nan)).astype(np.float32)
    valid = torch.isfinite(transform_fields(dev(up), dev(lat), scale=variant[0], rotation=variant[1])[1]).cpu().numpy()
    hb, wb = variant_size(variant)
    assert valid.shape == (hb, wb)
    off = (3, 5)
    ref = ref_composite(bg, obj, al, make_place(variant, off), 1.0, "hard", 1)
    got, cov = composite_objects(dev(bg), dev(obj), scale=variant[0], rotation=variant[1], offset=off, alpha=dev(al), edge="hard", return_coverage=True)
    sl = (slice(off[0], off[0] + hb), slice(off[1], off[1] + wb))
    sure = ~ref["borderline"][sl]
    assert np.array_equal((cov.cpu().numpy()[sl] > 0)[sure], valid[sure]) and set(np.unique(cov.cpu().numpy())) <= {0.0, 1.0}
    share = check(got, cov, ref, bg, "hard", str(variant))   # the colour is P / A
    print(f"{variant}: {int(valid.sum())} pixels pasted, {int((~sure).sum())} borderline, largest error / allowed {share[0]:.3f}")


def test_inactive_rows_return_the_background():
    from perspectivefields_amd import composite_objects

    nan = float("nan")
    for dtype in ("uint8", "float32"):
        bg, obj = picture("bg", dtype), picture("obj", dtype)
        if dtype == "float32":
            bg = with_nan_outside(bg, np.zeros(BG_HW, dtype=bool))
        rows = [(nan, 0.0, 3, 4, 15, 12), (0.0, 0.0, 3, 4, 15, 12), (1.0, 0.0, 3.5, 4, 15, 12), (1.0, 0.0, 45, 60, 15, 12), (1.0, 0.0, -15, 4, 15, 12),
                (1.0, nan, 3, 4, 15, 12), (1.0, 0.0, 3, 4, 0, 12), (nan, nan, -1, -1, -1, -1), (1.0, 0.0, 3, 4, 15, 12)]
        t = torch.tensor(rows, dtype=torch.float64, device="cuda")
        d_bg, d_obj = dev(bg), dev(obj)
        got, cov = composite_objects(d_bg, d_obj, pairs=[(0, 0)] * len(rows), scale=t[:, 0], rotation=t[:, 1], offset=t[:, 2:4], size=t[:, 4:6], return_coverage=True)
        assert got.shape == (len(rows),) + bg.shape and cov.shape == (len(rows),) + BG_HW
        for k in range(len(rows) - 1):
            assert same_bits(got[k], bg) and not cov[k].any(), (dtype, rows[k])
        assert not same_bits(got[-1], bg) and int((cov[-1] > 0).sum()) == 180   # the last row is active: the call did paste
        for row in rows[:5]:   # the same as host numbers
            one, c1 = composite_objects(d_bg, d_obj, scale=row[0], rotation=row[1], offset=row[2:4], size=row[4:6], return_coverage=True)
            assert same_bits(one, bg) and not c1.any(), (dtype, row)


def test_bits_do_not_depend_on_the_launch():
    """a job alone, in a batch of 33 (two launches), in a permuted batch, on a second run, and with its numbers as device tensors"""
    from perspectivefields_amd import composite_objects

    for dtype in ("uint8", "float32"):
        d_bg, d_obj, d_al = dev(picture("bg", dtype)), dev(picture("obj", dtype)), dev(alpha_plane("quarter"))
        jobs = [(VARIANTS[k % 7], (OFFSETS[k % 2][0] + k % 5, OFFSETS[k % 2][1] - k % 3)) for k in range(33)]
        cols = lambda idx: dict(scale=[jobs[k][0][0] for k in idx], rotation=[jobs[k][0][1] for k in idx], offset=[jobs[k][1] for k in idx],
                                size=[variant_size(jobs[k][0]) for k in idx])
        kw = dict(alpha=d_al, opacity=0.5, samples=2, return_coverage=True)
        order = list(range(33))
        batch, bcov = composite_objects(d_bg, d_obj, pairs=[(0, 0)] * 33, **cols(order), **kw)
        again, acov = composite_objects(d_bg, d_obj, pairs=[(0, 0)] * 33, **cols(order), **kw)
        assert same_bits(batch, again) and same_bits(bcov, acov)
        perm = [int(k) for k in np.random.default_rng(3).permutation(33)]
        mixed, mcov = composite_objects(d_bg, d_obj, pairs=[(0, 0)] * 33, **cols(perm), **kw)
        assert same_bits(mixed, batch[perm]) and same_bits(mcov, bcov[perm])
        as_t = {k: torch.tensor(v, dtype=torch.float64, device="cuda") for k, v in cols(order).items()}
        tens, tcov = composite_objects(d_bg, d_obj, pairs=[(0, 0)] * 33, **as_t, **kw)
        assert same_bits(tens, batch) and same_bits(tcov, bcov)
        for k in (0, 5, 31, 32):
            alone, c1 = composite_objects(d_bg, d_obj, **{n: v[0] for n, v in cols([k]).items()}, **kw)
            assert alone.shape == batch.shape[1:] and same_bits(alone, batch[k]) and same_bits(c1, bcov[k]), (dtype, k)
        assert len({batch[k].cpu().numpy().tobytes() for k in range(33)}) > 20   # the jobs differ


# ---------------------------------------------------------------- search -> paste
@functools.lru_cache(None)
def _planted_pictures():
    rng = np.random.default_rng(53)
    return (rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), [rng.integers(0, 256, (11, 10, 3), dtype=np.uint8), rng.integers(0, 256, (22, 19, 3), dtype=np.uint8)])


def test_the_chain_from_placement_search():
    from perspectivefields_amd import PerspectiveFields, composite_objects, placement_search

    up_bg, lat_bg, objs = planted_search()
    bg, pics = _planted_pictures()
    d_bg, d_pics = dev(bg), [dev(p) for p in pics]
    masks = [torch.isfinite(dev(o[1])) for o in objs]
    found = placement_search(dev(up_bg), dev(lat_bg), [dev(o[0]) for o in objs], [dev(o[1]) for o in objs], scales=PLANT_SCALES, rotations=PLANT_ROTATIONS)
    for kw in (dict(), dict(edge="hard", opacity=0.5, samples=2)):
        got, cov = PerspectiveFields.composite(None, d_bg, d_pics, found, alpha=masks, return_coverage=True, **kw)
        want, wcov = composite_objects(d_bg, d_pics, scale=[1.5, 0.75], rotation=[10.0, -10.0], offset=(12, 22), size=[(19, 18), (19, 17)], alpha=masks,
                                       return_coverage=True, **kw)
        assert got.shape == (2, 48, 64, 3) and same_bits(got, want) and same_bits(cov, wcov)
        assert all(int((cov[k] > 0).sum()) > 100 and not cov[k, :12].any() and not cov[k, :, :22].any() for k in range(2))
    one = PerspectiveFields.composite(None, d_bg, d_pics[0], found[0], alpha=masks[0])
    assert one.shape == (48, 64, 3) and same_bits(one, composite_objects(d_bg, d_pics[0], scale=1.5, rotation=10.0, offset=(12, 22), size=(19, 18), alpha=masks[0]))
    nothing = placement_search(dev(up_bg), dev(lat_bg), [dev(o[0]) for o in objs], [dev(o[1]) for o in objs], scales=(7.0, 9.0), rotations=(0.0, 90.0))
    assert all(int(d["best_variant"]) == -1 for d in nothing)
    got, cov = PerspectiveFields.composite(None, d_bg, d_pics, nothing, return_coverage=True)
    assert all(same_bits(got[k], bg) for k in range(2)) and not cov.any()


# ---------------------------------------------------------------- other forms of the arguments
def test_four_channel_object_and_lists_with_pairs():
    from perspectivefields_amd import composite_objects

    bg, obj = picture("bg", "uint8"), picture("obj", "uint8")
    a8 = (np.array(alpha_plane("quarter")) * 255).astype(np.uint8)   # 0, 63, 127, 191, 255
    rgba = np.concatenate([obj, a8[..., None]], axis=-1)
    kw = dict(scale=1.5, rotation=10.0, offset=(13, 22), samples=2)
    got, cov = composite_objects(dev(bg), dev(rgba), return_coverage=True, **kw)
    want = composite_objects(dev(bg), dev(obj), alpha=dev(a8.astype(np.float32)) / 255.0, **kw)
    assert same_bits(got, want)
    ref = ref_composite(bg, obj, (torch.from_numpy(a8.astype(np.float32)) / 255.0).numpy(), make_place((1.5, 10.0), (13, 22)), 1.0, "soft", 2)
    check(got, cov, ref, bg, "soft", "rgba")

    small = picture("bg", "uint8", (37, 53), 7)   # 37 x 53 x 3 bytes: the second image of a batch would not be aligned to 4 bytes, and 1961 pixels are no multiple of 4
    obj2 = picture("obj", "uint8", (9, 7), 9)
    bgs, objs = [dev(bg), dev(small)], [dev(obj), dev(obj2)]
    pairs = [(1, 0), (0, 1), (1, 1)]
    places = [make_place((0.75, -10.0), (20, 40)), (1.0, 90.0, 5.0, 6.0, 7.0, 9.0), (2.0, 0.0, -4.0, -3.0, 18.0, 14.0)]
    outs, covs = composite_objects(bgs, objs, pairs=pairs, scale=[p[0] for p in places], rotation=[p[1] for p in places], offset=[p[2:4] for p in places],
                                   size=[p[4:6] for p in places], return_coverage=True)
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(37, 53, 3), (40, 56, 3), (37, 53, 3)] and [tuple(c.shape) for c in covs] == [(37, 53), (40, 56), (37, 53)]
    for (b, o), place, out, cov in zip(pairs, places, outs, covs):
        hb = (bg, small)[b]
        ref = ref_composite(hb, (obj, obj2)[o], None, place)
        check(out, cov, ref, hb, "soft", str(place))
    # a batch tensor whose second image starts at an odd address: the channel-by-channel path gives the same bits
    batch = dev(np.stack([small, small]))
    two = composite_objects(batch, objs[1], scale=2.0, offset=(-4, -3), size=(18, 14))
    assert two.shape == (2, 37, 53, 3) and same_bits(two[0], outs[2]) and same_bits(two[1], outs[2])
