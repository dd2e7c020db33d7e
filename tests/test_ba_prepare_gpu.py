"""GPU: the two forms of RefineBA's graph construction (modules/sfm/reconstruction/BundleAdjuster.cpp:57-178) behind
eacham_ba_prepare — host loops (local windows) and device sorts + scans (eacham_amd/csrc/devprim.hpp, ba_prepare.hip) — must build
the SAME structure: every fp64 sum of the solver runs in the order of these lists, so the reduced system, the step and a
whole Levenberg-Marquardt run are compared BIT FOR BIT between a context forced to one form and a context forced to the
other (EACHAM_BA_PREPARE is read at eacham_ctx_create). Parity with the oracle is the business of tests/test_ba_gpu.py,
which runs on whichever form the problem size selects."""
import os

import numpy as np
import pytest

from eacham_amd import HipContext, ba, synth

pytestmark = pytest.mark.gpu


def _ctx_with(form, **env):
    """A context forced to one form of the construction (host | device), created under the given switches (they are read
    once, at eacham_ctx_create)."""
    env = dict(env, EACHAM_BA_PREPARE=form)
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return HipContext(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx_pair_with(**env):
    """(host-built, device-built) contexts created under the given switches."""
    host = _ctx_with("host", **env)
    try:
        return host, _ctx_with("device", **env)
    except BaseException:
        host.close()
        raise


@pytest.fixture(scope="module", params=["groups", "pairs"])
def ctx_pair(request):
    """(host-built, device-built) contexts under one form of the Schur stage: the landmark groups of csrc/ba_groups.hpp (what the
    device form builds by default) or the pair lists of rounds 1-4 (what the host form builds by default) — either form of the
    construction must reproduce either structure."""
    host, dev = _ctx_pair_with(EACHAM_BA_SCHUR=request.param)
    yield host, dev
    host.close()
    dev.close()


def _arrays(seed, n_cams, n_lm, k, shuffle=False, **kw):
    sc = synth.make_scene(n_cams, n_lm, k, seed=seed, **kw)
    A = ba.BaArrays.from_scene(sc)
    A.obs_uv[::13] += 30.0
    if shuffle:  # the caller's observation order is arbitrary: within a landmark it must be kept (a stable sort)
        perm = np.random.default_rng(seed).permutation(len(A.obs_cam))
        A.obs_cam, A.obs_point, A.obs_uv = A.obs_cam[perm].copy(), A.obs_point[perm].copy(), A.obs_uv[perm].copy()
    return A


def _same_structure(ctx_pair, A):
    host, dev = ctx_pair
    a, b = ba.PreparedBA(host, A), ba.PreparedBA(dev, A)
    try:
        for name in ba.PreparedBA.STRUCTURE:
            x, y = a.structure(name), b.structure(name)
            assert x.shape == y.shape and np.array_equal(x, y), f"structure array {name} differs ({x.shape} vs {y.shape})"
    finally:
        a.close()
        b.close()


def _same_step(ctx_pair, A, lam=1e-3):
    host, dev = ctx_pair
    _same_structure(ctx_pair, A)
    a = ba.debug_step(host, A, lam)
    b = ba.debug_step(dev, A, lam)
    for name, x, y in zip(["S", "g", "delta_c", "delta_l", "error", "lin_change"], a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), f"{name} differs between the host-built and the device-built structure"


def _same_run(ctx_pair, A, cfg=None):
    host, dev = ctx_pair
    cfg = cfg or ba.OptimizerConfig.refine_ba()
    a, b = ba.RefineBA(host, A, cfg), ba.RefineBA(dev, A, cfg)
    assert (a.outer_iterations, a.inner_iterations, a.status) == (b.outer_iterations, b.inner_iterations, b.status)
    assert a.initial_error == b.initial_error and a.final_error == b.final_error
    assert np.array_equal(a.trace, b.trace)
    assert np.array_equal(a.cam_T_wc, b.cam_T_wc) and np.array_equal(a.points, b.points) and np.array_equal(a.K, b.K)
    return a


@pytest.mark.parametrize("n_cams,n_lm,k,shuffle", [(5, 80, 3, False), (12, 300, 6, True), (31, 400, 6, False), (60, 600, 8, True),
                                                   (130, 2600, 6, True)])
def test_reduced_system_and_step_are_bit_identical(ctx_pair, n_cams, n_lm, k, shuffle):
    _same_step(ctx_pair, _arrays(7 + n_cams, n_cams, n_lm, k, shuffle=shuffle, pixel_noise=1.5))


def test_repeated_camera_unobserved_landmark_and_idle_camera(ctx_pair):
    A = _arrays(4, 6, 90, 3)
    # the same camera observes one landmark twice (two entries of its diagonal block per pair), an unobserved landmark
    # (an empty segment in the middle of lm_ptr), a camera nobody observes through (a diagonal block with no entry)
    A.obs_cam = np.concatenate([A.obs_cam, A.obs_cam[:5]]).astype(np.uint32)
    A.obs_point = np.concatenate([A.obs_point, A.obs_point[:5]]).astype(np.uint32)
    A.obs_uv = np.concatenate([A.obs_uv, A.obs_uv[:5] + 0.7])
    keep = A.obs_point != 17
    A.obs_cam, A.obs_point, A.obs_uv = A.obs_cam[keep].copy(), A.obs_point[keep].copy(), A.obs_uv[keep].copy()
    keep = A.obs_cam != 3
    A.obs_cam, A.obs_point, A.obs_uv = A.obs_cam[keep].copy(), A.obs_point[keep].copy(), A.obs_uv[keep].copy()
    _same_step(ctx_pair, A)
    _same_run(ctx_pair, A)


def test_whole_runs_are_bit_identical(ctx_pair):
    for A in [_arrays(21, 19, 1500, 7, shuffle=True, pixel_noise=1.0), _arrays(22, 130, 2600, 6, pixel_noise=1.0)]:
        out = _same_run(ctx_pair, A)
        assert out.outer_iterations >= 2 and out.final_error < out.initial_error
    _same_run(ctx_pair, _arrays(23, 40, 900, 6, pixel_noise=1.0), ba.OptimizerConfig("DogLeg", 30, 1e-5, 10.0, False))


def test_out_of_range_observation_is_refused_by_both(ctx_pair):
    from eacham_amd import EachamError, capi
    A = _arrays(5, 6, 90, 3)
    A.obs_point[11] = 90  # one past the last landmark
    for ctx in ctx_pair:
        with pytest.raises(EachamError) as e:
            ba.RefineBA(ctx, A, ba.OptimizerConfig.refine_ba())
        assert e.value.code == capi.ERR_INVALID


def test_metric_scene_is_bit_identical_and_reports_its_preparation(ctx_pair):
    """S200 (200 cameras / 50 000 landmarks / 500 000 observations): the size the device form is for."""
    host, dev = ctx_pair
    A = ba.BaArrays.from_scene(synth.make_scene(200, 50_000, 10, seed=12345))
    out = _same_run(ctx_pair, A)
    assert out.outer_iterations == 4
    infos = []
    for ctx in (host, dev):
        pb = ba.PreparedBA(ctx, A)
        infos.append(pb.plan_info())
        pb.close()
    assert infos[0]["panels"] == infos[1]["panels"] and infos[0]["tiles"] == infos[1]["tiles"] and infos[0]["levels"] == infos[1]["levels"]
    print("prepare_us host", infos[0]["prepare_us"], "device", infos[1]["prepare_us"])


@pytest.fixture(scope="module")
def config4_arrays():
    """BASELINE configs[3]: 500 cameras / 100 000 landmarks / 1 000 000 observations, built once for both forms of the Schur stage."""
    return ba.BaArrays.from_scene(synth.make_scene(500, 100_000, 10, seed=4))


def test_config4_is_bit_identical_and_plans_alike(ctx_pair, config4_arrays):
    """Config 4, five times the observations of S200: a whole run and the plan of the reduced camera system agree between the forms."""
    host, dev = ctx_pair
    out = _same_run(ctx_pair, config4_arrays)
    assert out.status == 0 and out.outer_iterations >= 2
    infos = []
    for ctx in (host, dev):
        pb = ba.PreparedBA(ctx, config4_arrays)
        infos.append(pb.plan_info())
        pb.close()
    for key in ("panels", "tiles", "levels", "ordering", "tile_updates"):
        assert infos[0][key] == infos[1][key], (key, infos)
    print("config 4 prepare_us host", infos[0]["prepare_us"], "device", infos[1]["prepare_us"])


def _group_rows(pb):
    """Rows per landmark group of a prepared problem; 0 when the pair lists serve."""
    n_groups = len(pb.structure("g_groups")) // 8
    return len(pb.structure("g_rowinfo")) // (2 * n_groups) if n_groups else 0


@pytest.mark.parametrize("rows", [16, 64, 252, 480, 508, 512])
def test_every_accepted_group_size_builds_the_same_structure(rows):
    """EACHAM_BA_GROUP_ROWS selects 16 to 508 rows per group (multiples of 4); 508 is the most the device form can pack
    (9-bit row fields of its entry keys, ba_prepare.hip prep_grp_entries). At every accepted size both forms of the construction
    choose the same structure and build it bit for bit alike; 512 is outside the range and ignored by both (the size the
    problem selects, 128 rows here, serves). At 16 rows a landmark of 8 observations (9 rows > 16 / 2) fits no group:
    both forms then take the pair lists."""
    pair = _ctx_pair_with(EACHAM_BA_SCHUR="groups", EACHAM_BA_GROUP_ROWS=str(rows))
    try:
        scenes = [_arrays(19, 12, 300, 6, shuffle=True, pixel_noise=1.5), _arrays(137, 130, 2600, 6, shuffle=True, pixel_noise=1.5)]
        if rows == 16:
            scenes.append(_arrays(67, 60, 600, 8, shuffle=True, pixel_noise=1.5))
        for i, A in enumerate(scenes):
            want = 0 if i == 2 else rows if rows <= 508 else 128
            got = []
            for ctx in pair:
                pb = ba.PreparedBA(ctx, A)
                got.append(_group_rows(pb))
                pb.close()
            assert got == [want, want], (rows, i, got)
            _same_step(pair, A)
        if rows in (16, 512):
            for A in scenes:
                _same_run(pair, A)
    finally:
        for ctx in pair:
            ctx.close()


@pytest.mark.parametrize("repeat", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("rows", [64, 252, 508])
def test_long_runs_cut_into_slices_and_segments_by_both_entry_kernels(rows, repeat):
    """Five cameras and three observations per landmark: a 508-row group holds about 120 landmarks, so a block's run inside a
    group is several slices long and the diagonal blocks exceed 64 entries — lanes are sliced, segments are cut at GRP_SEG
    lanes and some cross a row of GRP_ROW lanes. As it is the scene takes the sort-free entries kernel of ba_prepare.hip; with five
    observations repeated (a camera sees a landmark twice) every group goes through the general, sorting one. Both must
    build the host form's structure at every group size; `_group_rows` holds the case to the groups (not the pair lists)."""
    A = _arrays(31, 5, 300, 3)
    if repeat:
        A.obs_cam = np.concatenate([A.obs_cam, A.obs_cam[:5]]).astype(np.uint32)
        A.obs_point = np.concatenate([A.obs_point, A.obs_point[:5]]).astype(np.uint32)
        A.obs_uv = np.concatenate([A.obs_uv, A.obs_uv[:5] + 0.7])
    pair = _ctx_pair_with(EACHAM_BA_SCHUR="groups", EACHAM_BA_GROUP_ROWS=str(rows))
    try:
        for ctx in pair:
            pb = ba.PreparedBA(ctx, A)
            try:
                assert _group_rows(pb) == rows
            finally:
                pb.close()
        _same_step(pair, A)
        if rows == 508:
            _same_run(pair, A)
    finally:
        for ctx in pair:
            ctx.close()


def _same_bytes_as_a_fresh_host_build(dev, pb, A, env, lam=1e-3):
    """A problem prepared on the device-form context `dev` against the same problem on a FRESH context forced to the host form:
    all thirty structure arrays, the plan's panels / tiles / levels and one damped step, equal as bytes."""
    host = _ctx_with("host", **env)
    try:
        ref = ba.PreparedBA(host, A)
        try:
            for name in ba.PreparedBA.STRUCTURE:
                x, y = ref.structure(name), pb.structure(name)
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"structure array {name} differs ({x.shape} vs {y.shape})"
            want, got = ref.plan_info(), pb.plan_info()
            for key in ("panels", "tiles", "levels"):
                assert want[key] == got[key], (key, want, got)
        finally:
            ref.close()
        a, b = ba.debug_step(host, A, lam), ba.debug_step(dev, A, lam)
        for name, x, y in zip(["S", "g", "delta_c", "delta_l", "error", "lin_change"], a, b):
            assert np.asarray(x, np.float64).tobytes() == np.asarray(y, np.float64).tobytes(), f"{name} differs from the host-built problem's"
    finally:
        host.close()


@pytest.mark.parametrize("schur", ["groups", "pairs"])
def test_device_built_problems_keep_their_bytes_under_reuse_of_both_arenas(schur):
    """A device-built problem lives in two arenas of the context's pool (csrc/ba_prepare.hip: what (cameras, landmarks,
    observations) size, then what the pair lists / groups and the plan size). On ONE context: two problems alive together, one
    released, a refused problem (an observation names camera n_cams: the call leaves after the first arena was taken and must
    give back what it holds), a third problem of the released one's size (it is carved out of the released blocks, which hold
    the old problem's bytes), the first once more. Every prepared problem must be the host-built one byte for byte."""
    from eacham_amd import EachamError, capi
    env = {"EACHAM_BA_SCHUR": schur}
    A, B, C = _arrays(41, 6, 90, 3), _arrays(42, 12, 300, 6, shuffle=True), _arrays(43, 6, 90, 3)
    dev = _ctx_with("device", **env)
    alive = []
    try:
        pa, pb = ba.PreparedBA(dev, A), ba.PreparedBA(dev, B)
        alive += [pa, pb]
        _same_bytes_as_a_fresh_host_build(dev, pa, A, env)
        _same_bytes_as_a_fresh_host_build(dev, pb, B, env)
        pa.close()
        bad = _arrays(41, 6, 90, 3)
        bad.obs_cam[11] = 6  # camera n_cams
        with pytest.raises(EachamError) as e:
            ba.PreparedBA(dev, bad)
        assert e.value.code == capi.ERR_INVALID
        pc = ba.PreparedBA(dev, C)
        alive.append(pc)
        _same_bytes_as_a_fresh_host_build(dev, pc, C, env)
        pa2 = ba.PreparedBA(dev, A)
        alive.append(pa2)
        _same_bytes_as_a_fresh_host_build(dev, pa2, A, env)
        _same_bytes_as_a_fresh_host_build(dev, pb, B, env)  # (untouched by what came and went beside it)
    finally:
        for p in alive:
            p.close()
        dev.close()
