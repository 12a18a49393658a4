"""Shapes, channel forms and usability-query forms of tests/test_gpu_conv_forms.py, and the plain launches (groups = 1, ups = 0) it makes with a named tile -- kept
apart from the test module so that tests/test_gpu_ops.py::test_every_conv_tile_is_run_by_a_case_that_names_it can count them without importing another test module.
Plain data and host logic: nothing here touches a device, and nothing is evaluated at import."""

# (B, H, W), the full-resolution size (even, for the up-sampling forms)
SHAPES = [
    (1, 2, 2),     # a 1 x 1 source: every tap clamps; every pixel is a corner
    (2, 6, 10),    # odd half-resolution size 3 x 5; ragged against 8 x 16 and 16 x 16 patches
    (1, 18, 34),   # crosses patch boundaries in both directions, ragged last patch for either patch size
    (3, 16, 32),   # exact multiples
]
GROUP_SHAPES = SHAPES + [(1, 10, 10)]  # 100 rows: group 0's last tile is ragged, group 1 starts inside what a 128-row tile would cover
TABLE_SHAPES = [(2, 2, 2), (1, 2, 5), (1, 3, 3), (2, 10, 12)]

# name -> C1, C2, Cout, act: the up-sampling forms (conv_fuse_conv1 is 64 -> 32 + ReLU, conv_fuse_conv0 the concat form)
UPS_FORMS = {"ups64-32": (64, 0, 32, 1), "ups32-64": (32, 0, 64, 0), "ups32-128": (32, 0, 128, 0), "ups64+32-64": (64, 32, 64, 0)}
# name -> C1, Cout, K, pad, act, residuals, post_relu, shapes: the grouped forms
GROUP_FORMS = {
    "r1c2": (64, 64, 3, 1, 0, 2, True, GROUP_SHAPES),     # ResidualConvUnit conv2 with the fusion add: two residuals, ReLU behind them
    "relu": (64, 64, 3, 1, 1, 0, False, GROUP_SHAPES),
    "mlp1x1": (64, 96, 1, 0, 0, 0, False, [(1, 100, 1)]),  # the decoders' MLP: 100 rows, ragged against every row tile, 96 columns against 64 / 128
    "wino": (64, 64, 3, 1, 0, 0, False, GROUP_SHAPES),     # the plain Winograd-eligible form
}
# name -> C1, Cout: the bias-table forms (3 x 3 / pad 1).  40: a ragged last column tile; 38: no multiple of 4, the scalar tail of the epilogues
TABLE_FORMS = {"tab32-64": (32, 64), "tab32-40": (32, 40), "tab32-38": (32, 38)}

# the forms the tile lists are asked for (ops.conv2d_g_tiles); the answer does not depend on the map size (test_tile_lists_hold_the_families_the_engine_uses)
Q_UPS = dict(B=2, H=6, W=10, C1=64, Cout=32, K=3, pad=1, ups=True)
Q_UPS_HEAD = dict(B=2, H=6, W=10, C1=64, Cout=32, K=3, pad=1, act=1, ups=True, head_kind=1)
Q_GROUP3 = dict(B=1, H=10, W=10, C1=64, Cout=64, K=3, pad=1, groups=2)
Q_GROUP1 = dict(B=1, H=100, W=1, C1=64, Cout=96, K=1, groups=2)
Q_GROUP_HEAD = dict(B=1, H=10, W=10, C1=64, Cout=32, K=3, pad=1, act=1, groups=2, head_kind=1)
Q_SPLITK = dict(B=1, H=10, W=10, C1=128, Cout=64, K=3, pad=1, groups=2)
Q_TABLE = dict(B=1, H=3, W=3, C1=32, Cout=64, K=3, pad=1, has_table=True)


def is_linear_sb(name):
    return name.startswith("sb") and not name.startswith("sbh")


def plain_conv_cases(ops):
    """the groups = 1, ups = 0 launches of tests/test_gpu_conv_forms.py that name a tile: [(case, tile names)], the case in the layout of
    tests/test_gpu_ops.py::CONV_CASES (name, B, H, W, C1, C2, Cout, K, stride, pad) -- the materialised side of the up-sampling identity (ops.conv2d on the up-sampling
    tiles) and the single-problem side of the grouped identities (ops.conv2d_g, which refuses a tile it cannot run).  `ops`: perspectivefields_amd.ops; a library that
    cannot be loaded raises here."""
    names = ops.conv_tiles()
    ups, g3, g1 = ([names[t] for t in ops.conv2d_g_tiles(**q)] for q in (Q_UPS, Q_GROUP3, Q_GROUP1))
    cases = []
    for name, (C1, C2, Cout, _) in UPS_FORMS.items():
        cases += [((f"{name}@{B}x{H}x{W}", B, H, W, C1, C2, Cout, 3, 1, 1), ups) for B, H, W in SHAPES]
    for name, (C1, Cout, K, pad, _, _, _, shapes) in GROUP_FORMS.items():
        cases += [((f"{name}@{B}x{H}x{W}", B, H, W, C1, 0, Cout, K, 1, pad), g3 if K == 3 else g1) for B, H, W in shapes]
    return cases + [(("splitk128-64@1x10x10", 1, 10, 10, 128, 0, 64, 3, 1, 1), [n for n in names if is_linear_sb(n)])]
