"""Helpers shared by the GPU parity suites (tests/test_gpu_parity.py, tests/test_gpu_alloc_ties.py):
the allocator variants' environment knobs, a handle on device 0 and the lockstep run against the C
oracle. Bar: bit-exact integer state, observations and PCG64 states; rewards within 1e-6 absolute."""
import numpy as np
import torch

import oracle as orc

REW_ATOL = 1e-6


def _set_alloc(monkeypatch, param):
    # "<impl>[_<opt>...]": impl lane / lane2 / lane4 (one env per lane, 1 / 2 / 4 lanes per env),
    # group (one env per lane group), scan (one env per wave, prefix scan over the cost ranking);
    # opts sorted / unsorted (group kernel's visiting order), ea0 / ea1 (episode-ahead demand off /
    # on; default: on for the scan kernel, the library's choice for group, off for lane), nofc (the
    # scan allocator without its fused phases A and C: the step_a / step_c kernels run), nofa (phase C
    # fused, phase A in step_a)
    impl, *opts = param.split("_")
    monkeypatch.setenv("MSC_ALLOC_IMPL", "lane" if impl.startswith("lane") else impl)
    monkeypatch.setenv("MSC_ALLOC_LPE", impl[4:] if impl.startswith("lane") and impl[4:] else "0")
    # group kernel: envs visited in descending order of their order count (default for empirical
    # demand), forced on ("sorted") or off ("unsorted")
    sort = [o for o in opts if o in ("sorted", "unsorted")]
    if sort:
        monkeypatch.setenv("MSC_ALLOC_SORT", "1" if sort[0] == "sorted" else "0")
    else:
        monkeypatch.delenv("MSC_ALLOC_SORT", raising=False)
    # step_a / step_c with the pending ring in registers: off with the lane kernel (as the library
    # runs at >= 16,384 envs, C3), on with the others (its default below that), so both forms of the
    # two phase kernels meet every reference
    monkeypatch.setenv("MSC_OBS_RING_REG", "0" if impl.startswith("lane") else "1")
    # step_c's observation stage: the library's choice with the lane kernel (two phases; off with
    # episode-ahead demand, as with scan), the whole block in one phase with the group kernel
    if impl == "group":
        monkeypatch.setenv("MSC_OBS_STAGE", "1")
    else:
        monkeypatch.delenv("MSC_OBS_STAGE", raising=False)
    # the scan allocator runs phase C itself (MSC_FUSE_C, default on); "nofc" keeps the step_c kernel
    if "nofc" in opts:
        monkeypatch.setenv("MSC_FUSE_C", "0")
    else:
        monkeypatch.delenv("MSC_FUSE_C", raising=False)
    if "nofa" in opts:  # phase C fused, phase A in the step_a kernel
        monkeypatch.setenv("MSC_FUSE_A", "0")
    else:
        monkeypatch.delenv("MSC_FUSE_A", raising=False)
    ea = "0" if "ea0" in opts or impl.startswith("lane") else "1" if ("ea1" in opts or impl == "scan") else None
    if ea is None:
        monkeypatch.delenv("MSC_EA", raising=False)
    else:
        monkeypatch.setenv("MSC_EA", ea)


def _vec(spec, E, **kw):
    from marlsc.vec_env import VecInventoryEnv
    return VecInventoryEnv(None, E, spec=spec, device=0, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _lockstep(spec, E, steps, seed=0, base_seed=777, check_every=1):
    env = _vec(spec, E, base_seed=base_seed)
    ref = orc.OracleEnv(spec, E, base_seed=base_seed)
    np.testing.assert_array_equal(_np(env.reset()), ref.reset())
    rng = np.random.default_rng(seed)
    for t in range(steps):
        a = rng.uniform(-1, 1, size=(E, spec.W, spec.K)).astype(np.float32)
        og, _, tg, fg = env.step(torch.from_numpy(a).cuda(), want_f64=True)
        orr, rr, tr, fr = ref.step(a, final_obs=True, n_threads=8)
        assert np.array_equal(_np(tg).astype(bool), tr)
        np.testing.assert_allclose(_np(env.rewards_f64), rr, rtol=0, atol=REW_ATOL, err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(og), orr, err_msg=f"obs t={t}")
        if tr.any():
            np.testing.assert_array_equal(_np(fg)[tr], fr[tr], err_msg=f"final obs t={t}")
        if t % check_every == 0:
            sg, sr = env.read_state(), ref.read_state()
            np.testing.assert_array_equal(sg["inventory"], sr["inventory"])
            np.testing.assert_array_equal(sg["rng"], sr["rng"])
            np.testing.assert_array_equal(sg["timestep"], sr["timestep"])
    env.check()
    return env, ref
