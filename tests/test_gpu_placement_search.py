"""Similarity transforms of perspective fields and the placement search on the GPU (include/pf_hip.h pf_fields_transform, pf_place_search;
perspectivefields_amd.transform_fields, placement_search, PerspectiveFields.placement_search) against the fp64 reference of
tests/test_placement_search_ref.py on its fixed inputs, the bit identities that tie the search to transform_fields + placement_scores, the planted
search, determinism, thresholds and weights, and the model method.

Tolerances (derived in the reference file's docstring, not fitted): per pixel the fp32 source position's error bound times the
largest difference among the pixel's taps, plus 4 x 2^-24 for the up vector's components (fp32 cos and sin, one rounding) and one rounding of the
latitude.  Validity must be equal outside borderline pixels (|W_v - 1/2| < 1e-3), which are left out of both comparisons.  The output up vectors have
unit length to 2 ulp.  The search's numbers are held to the composition transform_fields + placement_scores + torch minima BIT FOR BIT; only the
planted search is compared with the reference's numbers, to the bound the reference derives."""
import functools

import numpy as np
import pytest
import torch

from tests.test_placement_ref import BG_CAM, camera_fields, crop, ellipse
from tests.test_placement_search_ref import (PLANT_ROTATIONS, PLANT_SCALES, planted_search, ref_search, ref_transform, search_set, set_search_reference,
                                             transform_cases, variant_list)

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
KEYS = ("pfd_deg", "up_mean_deg", "lat_mean_deg", "valid_pixels", "best_offset", "best_pfd_deg")
OUT = ("best_scale", "best_rotation_deg", "best_variant", "best_offset", "best_pfd_deg", "best_up_mean_deg", "best_lat_mean_deg", "best_size", "variant_pfd_deg",
       "variant_offset", "variant_size", "variant_valid_pixels")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the cached inputs are read-only


def same_bits(a, b):
    a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_transform(got, ref, what):
    """(up', lat') of the device against ref_transform's dict; returns the largest error as a share of the allowed: (up, latitude)"""
    up, lat = (t.cpu().numpy() for t in got)
    assert up.dtype == np.float32 and lat.dtype == np.float32 and up.shape == ref["up"].shape and lat.shape == ref["lat"].shape, what
    valid = ~np.isnan(lat)
    assert np.array_equal(np.isnan(up[0]), ~valid) and np.array_equal(np.isnan(up[1]), ~valid), what   # NaN in all three planes or in none
    sure = ~ref["borderline"]
    assert np.array_equal(valid[sure], ref["valid"][sure]), (what, int((valid != ref["valid"])[sure].sum()))
    cmp = valid & ref["valid"] & sure
    if not cmp.any():
        return 0.0, 0.0
    e_up = np.abs(up.astype(np.float64) - ref["up"]).max(0)[cmp]
    e_lat = np.abs(lat.astype(np.float64) - ref["lat"])[cmp]
    share = float((e_up / ref["tol_up"][cmp]).max()), float((e_lat / np.maximum(ref["tol_lat"][cmp], 1e-300)).max())
    assert (e_up <= ref["tol_up"][cmp]).all() and (e_lat <= ref["tol_lat"][cmp]).all(), (what, e_up.max(), e_lat.max(), share)
    length = np.hypot(up[0].astype(np.float64), up[1].astype(np.float64))[valid]
    assert np.abs(length - 1.0).max() <= 2 * ULP, (what, np.abs(length - 1.0).max())
    return share


def noisy_object(h=9, w=7, seed=11, holes=True):
    up, lat = crop(*camera_fields(*BG_CAM, 40, 56, seed=seed), 5, 6, h, w)
    if holes:
        lat[1 % h, 2 % w] = np.nan
        up[:, h // 2, w // 2] = 0.0
    return up, lat


# ---------------------------------------------------------------- transform_fields against the reference
def test_fixed_variants_match_the_reference_with_and_without_mask():
    from perspectivefields_amd import transform_fields

    worst = {}
    groups = {}
    for name, u, l, s, r in transform_cases():
        groups.setdefault(name, (u, l, []))[2].append((s, r))
    for name, (u, l, variants) in groups.items():
        sc, ro = [v[0] for v in variants], [v[1] for v in variants]
        got = transform_fields(dev(u), dev(l), scale=sc, rotation=ro)
        m = ellipse(*l.shape)
        masked = transform_fields(dev(u), dev(l), scale=sc, rotation=ro, mask=dev(m))
        assert isinstance(got, list) and len(got) == len(variants)
        for (s, r), g, gm in zip(variants, got, masked):
            a = check_transform(g, ref_transform(u, l, s, r), f"{name} ({s}, {r})")
            b = check_transform(gm, ref_transform(u, np.where(m, l, np.nan).astype(np.float32), s, r), f"{name} ({s}, {r}) masked")
            worst[name] = tuple(max(x) for x in zip(worst.get(name, (0.0, 0.0)), a, b))
    for name, (a, b) in worst.items():
        print(f"{name}: largest error / allowed: up {a:.3f}, latitude {b:.3f}")


def test_small_objects_scales_rotations_and_two_launches():
    from perspectivefields_amd import transform_fields

    variants = variant_list((0.5, 0.75, 1.5, 2.0), (0.0, 10.0, -10.0, 90.0, 137.0))
    worst = (0.0, 0.0)
    for what, (u, l) in (("1 x 1", noisy_object(1, 1, holes=False)), ("2 x 3", noisy_object(2, 3, holes=False)), ("9 x 7", noisy_object())):
        got = transform_fields(dev(u), dev(l), scale=[v[0] for v in variants], rotation=[v[1] for v in variants])
        for (s, r), g in zip(variants, got):
            worst = tuple(max(x) for x in zip(worst, check_transform(g, ref_transform(u, l, s, r), f"{what} ({s}, {r})")))
    # 33 variants in one call: two launches; a given size
    u, l = noisy_object(12, 10, seed=12)
    many = [(0.5 + 0.05 * k, -40.0 + 7.0 * k) for k in range(33)]
    got = transform_fields(dev(u), dev(l), scale=[v[0] for v in many], rotation=[v[1] for v in many])
    for (s, r), g in zip(many, got):
        worst = tuple(max(x) for x in zip(worst, check_transform(g, ref_transform(u, l, s, r), f"12 x 10 ({s}, {r})")))
    g = transform_fields(dev(u), dev(l), scale=1.25, rotation=20.0, height=9, width=21)
    worst = tuple(max(x) for x in zip(worst, check_transform(g, ref_transform(u, l, 1.25, 20.0, height=9, width=21), "given size")))
    print(f"largest error / allowed: up {worst[0]:.3f}, latitude {worst[1]:.3f}")
    # several fields in one call
    both = transform_fields([dev(u), dev(noisy_object()[0])], [dev(l), dev(noisy_object()[1])], scale=1.5, rotation=-10.0)
    assert same_bits(both[0][0], transform_fields(dev(u), dev(l), scale=1.5, rotation=-10.0)[0])
    check_transform(both[1], ref_transform(*noisy_object(), 1.5, -10.0), "second field")


# ---------------------------------------------------------------- bit identities
def test_identity_returns_the_bits_and_half_turns_undo_each_other():
    from perspectivefields_amd import transform_fields
    from tests.test_placement_ref import field_valid

    u, l = noisy_object()
    keep = field_valid(u, l)
    up, lat = (t.cpu().numpy() for t in transform_fields(dev(u), dev(l)))
    assert same_bits(up[:, keep], u[:, keep]) and same_bits(lat[keep], l[keep]) and np.isnan(up[:, ~keep]).all() and np.isnan(lat[~keep]).all()
    once = transform_fields(dev(u), dev(l), rotation=180.0)
    up, lat = (t.cpu().numpy() for t in transform_fields(*once, rotation=-180.0))
    assert np.array_equal(up[:, keep], u[:, keep]) and np.array_equal(lat[keep], l[keep]) and np.isnan(lat[~keep]).all()
    quarter = transform_fields(dev(u), dev(l), rotation=90.0)
    assert tuple(quarter[1].shape) == (7, 9)
    r = ref_transform(u, l, 1.0, 90.0)
    assert np.array_equal(quarter[1].cpu().numpy(), r["lat"].astype(np.float32), equal_nan=True)   # a permutation of the pixels: exact
    assert np.array_equal(quarter[0].cpu().numpy(), r["up"].astype(np.float32), equal_nan=True)


def test_a_variant_has_the_same_bits_alone_in_a_batch_permuted_and_again():
    from perspectivefields_amd import transform_fields

    u, l = noisy_object(12, 10, seed=12)
    du, dl = dev(u), dev(l)
    many = [(0.5 + 0.05 * k, -40.0 + 7.0 * k) for k in range(33)]
    batch = transform_fields(du, dl, scale=[v[0] for v in many], rotation=[v[1] for v in many])
    again = transform_fields(du, dl, scale=[v[0] for v in many], rotation=[v[1] for v in many])
    perm = np.random.default_rng(5).permutation(33)
    mixed = transform_fields(du, dl, scale=[many[k][0] for k in perm], rotation=[many[k][1] for k in perm])
    for k in (0, 7, 31, 32):
        alone = transform_fields(du, dl, scale=many[k][0], rotation=many[k][1])
        assert same_bits(alone[0], batch[k][0]) and same_bits(alone[1], batch[k][1]), k
    for k in range(33):
        assert same_bits(batch[k][0], again[k][0]) and same_bits(batch[k][1], again[k][1]), k
        assert same_bits(batch[perm[k]][0], mixed[k][0]) and same_bits(batch[perm[k]][1], mixed[k][1]), k


def compose(up_bg, lat_bg, up_obj, lat_obj, variants, mask=None, **kw):
    """what a caller composes from transform_fields, placement_scores and torch minima: (per variant the placement_scores dict or None, the entries
    placement_search derives).  The first minimum in variant order, then in row-major order (placement_scores' own)."""
    from perspectivefields_amd import placement_scores, transform_fields

    tf = transform_fields(up_obj, lat_obj, scale=[v[0] for v in variants], rotation=[v[1] for v in variants], mask=mask)
    H, W = lat_bg.shape
    maps = [placement_scores(up_bg, lat_bg, tu, tl, **kw) if tl.shape[0] <= H and tl.shape[1] <= W else None for tu, tl in tf]
    pfd = torch.stack([torch.tensor(float("inf"), dtype=torch.float64, device="cuda") if m is None else m["best_pfd_deg"] for m in maps])
    off = torch.stack([torch.full((2,), -1, dtype=torch.int64, device="cuda") if m is None else m["best_offset"] for m in maps])
    size = torch.tensor([tuple(tl.shape) for _, tl in tf], dtype=torch.int64, device="cuda")
    valid = torch.stack([(torch.isfinite(tl) & torch.isfinite(tu).all(0)).sum() for tu, tl in tf])
    v = int(torch.argmin(pfd)) if bool(torch.isfinite(pfd).any()) else -1
    v = -1 if v < 0 else int(torch.nonzero(pfd == pfd.min())[0])   # the first of equal minima
    nan = torch.tensor(float("nan"), dtype=torch.float64, device="cuda")
    out = dict(variant_pfd_deg=pfd, variant_offset=off, variant_size=size, variant_valid_pixels=valid, best_variant=torch.tensor(v, device="cuda"),
               best_pfd_deg=pfd[v] if v >= 0 else pfd[0], best_offset=off[v] if v >= 0 else off[0] * 0 - 1,
               best_size=size[v] if v >= 0 else size[0] * 0 - 1,
               best_scale=torch.tensor(variants[v][0] if v >= 0 else float("nan"), dtype=torch.float64, device="cuda"),
               best_rotation_deg=torch.tensor(variants[v][1] if v >= 0 else float("nan"), dtype=torch.float64, device="cuda"))
    if v >= 0:
        j, i = (int(x) // maps[v]["stride"] for x in off[v])
        out.update(best_up_mean_deg=maps[v]["up_mean_deg"][j, i], best_lat_mean_deg=maps[v]["lat_mean_deg"][j, i])
    else:
        out.update(best_up_mean_deg=nan, best_lat_mean_deg=nan)
    return maps, out


def check_against_composition(got, up_bg, lat_bg, up_obj, lat_obj, variants, what, **kw):
    maps, want = compose(up_bg, lat_bg, up_obj, lat_obj, variants, **kw)
    for k in OUT:
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])
    if "maps" in got:
        assert len(got["maps"]) == len(maps)
        for v, (g, w) in enumerate(zip(got["maps"], maps)):
            assert (g is None) == (w is None), (what, v)
            if g is not None:
                for k in KEYS:
                    assert same_bits(g[k], w[k]), (what, v, k)


@functools.lru_cache(None)
def set_results(name):
    from perspectivefields_amd import placement_search

    bgs, objs, pairs, scales, rots, stride = search_set(name)
    d_bgs, d_objs = [(dev(u), dev(l)) for u, l in bgs], [(dev(u), dev(l)) for u, l in objs]
    res = placement_search([b[0] for b in d_bgs], [b[1] for b in d_bgs], [o[0] for o in d_objs], [o[1] for o in d_objs], scales=scales, rotations=rots,
                           pairs=pairs, stride=stride, return_maps=True)
    assert isinstance(res, list) and len(res) == len(pairs)
    return d_bgs, d_objs, res


@pytest.mark.parametrize("name", list("GHI"))
def test_search_equals_the_composition_bit_for_bit(name):
    _, _, pairs, scales, rots, stride = search_set(name)
    d_bgs, d_objs, res = set_results(name)
    variants = variant_list(scales, rots)
    for (b, o), got, ref in zip(pairs, res, set_search_reference(name)):
        for k in OUT:
            assert got[k].is_cuda and got[k].dtype == (torch.float64 if k.endswith("_deg") or k == "best_scale" else torch.int64), k
        check_against_composition(got, *d_bgs[b], *d_objs[o], variants, f"set {name} pair ({b}, {o})", stride=stride)
        # and the reference's winner: the sets are determined (asserted in the reference file)
        assert int(got["best_variant"]) == ref["best_variant"] and tuple(got["best_offset"].tolist()) == ref["best_offset"]
        assert abs(float(got["best_pfd_deg"]) - ref["best_pfd_deg"]) <= ref["bound"][ref["best_variant"]]
        assert [tuple(x) for x in got["variant_size"].tolist()] == ref["size"] and got["variant_valid_pixels"].tolist() == ref["valid_pixels"]
        for v, m in enumerate(ref["maps"]):
            assert (got["maps"][v] is None) == (m is None)
            if m is None:
                assert float(got["variant_pfd_deg"][v]) == float("inf") and got["variant_offset"][v].tolist() == [-1, -1]


def test_planted_search_finds_scale_rotation_and_offset():
    from perspectivefields_amd import placement_search

    up_bg, lat_bg, objs = planted_search()
    variants = variant_list(PLANT_SCALES, PLANT_ROTATIONS)
    d_bg = (dev(up_bg), dev(lat_bg))
    both = placement_search(*d_bg, [dev(o[0]) for o in objs], [dev(o[1]) for o in objs], scales=PLANT_SCALES, rotations=PLANT_ROTATIONS, return_maps=True)
    for (up_obj, lat_obj), got, want, size in zip(objs, both, ((1.5, 10.0), (0.75, -10.0)), ((19, 18), (19, 17))):
        ref = ref_search(up_bg, lat_bg, up_obj, lat_obj, variants)
        v = ref["best_variant"]
        assert variants[v] == want and ref["size"][v] == size
        assert int(got["best_variant"]) == v and (float(got["best_scale"]), float(got["best_rotation_deg"])) == want
        assert got["best_offset"].tolist() == [12, 22] and tuple(got["best_size"].tolist()) == size
        err = abs(float(got["best_pfd_deg"]) - ref["best_pfd_deg"])
        print(f"object {lat_obj.shape}: best PFD {float(got['best_pfd_deg']):.4f} deg, reference {ref['best_pfd_deg']:.4f}, error {err:.2e} of {ref['bound'][v]:.2e} allowed")
        assert err <= ref["bound"][v]
        assert [tuple(x) for x in got["variant_size"].tolist()] == ref["size"]
        check_against_composition(got, *d_bg, dev(up_obj), dev(lat_obj), variants, f"planted {lat_obj.shape}")


# ---------------------------------------------------------------- determinism
def _all_bits(d):
    out = [d[k] for k in OUT]
    for m in d.get("maps", []):
        if m is not None:
            out += [m[k] for k in KEYS]
    return out


def test_results_do_not_depend_on_the_run_the_batch_or_the_order():
    from perspectivefields_amd import placement_search

    _, _, pairs, scales, rots, stride = search_set("I")
    d_bgs, d_objs, res = set_results("I")
    args = ([b[0] for b in d_bgs], [b[1] for b in d_bgs], [o[0] for o in d_objs], [o[1] for o in d_objs])
    kw = dict(scales=scales, rotations=rots, stride=stride, return_maps=True)
    again = placement_search(*args, pairs=pairs, **kw)
    order = [2, 0, 1]
    mixed = placement_search(*args, pairs=[pairs[k] for k in order], **kw)
    for k, (b, o) in enumerate(pairs):
        alone = placement_search(*d_bgs[b], *d_objs[o], **kw)
        assert isinstance(alone, dict)
        for x, y, z, w in zip(_all_bits(res[k]), _all_bits(again[k]), _all_bits(alone), _all_bits(mixed[order.index(k)])):
            assert same_bits(x, y) and same_bits(x, z) and same_bits(x, w), (k, b, o)


# ---------------------------------------------------------------- thresholds, weights, empty results
@pytest.mark.parametrize("min_valid", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (2.0, 0.5), (0.0, 1.0)])
def test_thresholds_and_weights_follow_the_composition(min_valid, weights):
    from perspectivefields_amd import placement_search

    bgs, objs, _, _, _, _ = search_set("I")
    up_bg, lat_bg = np.array(bgs[0][0]), np.array(bgs[0][1])
    lat_bg[10:15, :] = np.nan   # placements with fewer valid pairs: the threshold decides
    lat_bg[:6, :6] = np.nan
    d_bg, d_obj = (dev(up_bg), dev(lat_bg)), (dev(objs[1][0]), dev(objs[1][1]))
    variants = variant_list((0.75, 1.5), (-10.0, 10.0))
    got = placement_search(*d_bg, *d_obj, scales=(0.75, 1.5), rotations=(-10.0, 10.0), stride=2, min_valid=min_valid, weights=weights, return_maps=True)
    check_against_composition(got, *d_bg, *d_obj, variants, f"min_valid {min_valid}, weights {weights}", stride=2, min_valid=min_valid, weights=weights)
    inf = sum(int(torch.isinf(m["pfd_deg"]).sum()) for m in got["maps"])
    assert (inf == 0) == (min_valid == 0.0)


def test_nothing_to_find_gives_inf_and_minus_one():
    from perspectivefields_amd import placement_search

    bgs, objs, _, _, _, _ = search_set("G")
    d_bg = (dev(bgs[0][0]), dev(bgs[0][1]))
    u, l = objs[0]
    for what, got in (("all NaN", placement_search(*d_bg, dev(u), dev(np.full_like(l, np.nan)), scales=(0.75, 1.5), rotations=(0.0, 10.0), min_valid=0.0)),
                      ("masked out", placement_search(*d_bg, dev(u), dev(l), scales=(1.0,), mask=torch.zeros(l.shape, dtype=torch.bool, device="cuda"))),
                      ("too large", placement_search(*d_bg, dev(u), dev(l), scales=(7.0, 9.0), rotations=(0.0, 90.0)))):
        assert float(got["best_pfd_deg"]) == float("inf") and int(got["best_variant"]) == -1 and got["best_offset"].tolist() == [-1, -1], what
        assert got["best_size"].tolist() == [-1, -1] and np.isnan(float(got["best_scale"])) and np.isnan(float(got["best_up_mean_deg"])), what
        assert torch.isinf(got["variant_pfd_deg"]).all() and (got["variant_offset"] == -1).all(), what
        if what != "too large":
            assert (got["variant_valid_pixels"] == 0).all(), what
        else:
            assert got["variant_size"].tolist() == [[63, 49], [49, 63], [81, 63], [63, 81]] and (got["variant_valid_pixels"] > 0).all()


# ---------------------------------------------------------------- the model method
def test_model_method_equals_the_function():
    from perspectivefields_amd import PerspectiveFields, placement_search

    rng = np.random.default_rng(21)
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    bg = m.inference_batch([rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)])
    obj = m.inference_batch([rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)])
    kw = dict(scales=(0.75, 1.5), rotations=(-10.0, 10.0), stride=4)
    got = m.placement_search(bg[0], obj[0], **kw)
    want = placement_search(bg[0]["pred_gravity_original"], bg[0]["pred_latitude_original"], obj[0]["pred_gravity_original"], obj[0]["pred_latitude_original"], **kw)
    assert isinstance(got, dict) and got["variant_pfd_deg"].shape == (4,) and got["stride"] == 4
    assert all(same_bits(got[k], want[k]) for k in OUT)
    assert torch.isfinite(got["best_pfd_deg"]) and int(got["best_offset"][0]) % 4 == 0 and 0 <= int(got["best_variant"]) < 4
    lists = m.placement_search(bg, obj, **kw)
    assert isinstance(lists, list) and len(lists) == 1 and all(same_bits(lists[0][k], want[k]) for k in OUT)
