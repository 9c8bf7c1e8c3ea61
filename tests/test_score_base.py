"""prediff_amd.score_base: what the four SEVIR score classes inherit -- the constructor contract, sync() with a rank that made no
update (two gloo processes on the CPU), the workspace rule and the names sevir_skill.py still exports.  Host only."""
import os
import socket

import numpy as np
import pytest
import torch

CLASSES = ("SEVIRSkillScore", "SEVIREnsembleScore", "SEVIRFrameScore", "SEVIRSpectralScore")
SEQ_LEN_ERROR = {"SEVIRSkillScore": AssertionError, "SEVIREnsembleScore": AssertionError, "SEVIRFrameScore": ValueError,
                 "SEVIRSpectralScore": ValueError}
LAYOUT_CHECKED = CLASSES[1:]         # SEVIRSkillScore takes a layout as the reference class does
HW = (8, 12)


def score_class(name):
    from prediff_amd.ensemble_score import SEVIREnsembleScore
    from prediff_amd.frame_score import SEVIRFrameScore
    from prediff_amd.sevir_skill import SEVIRSkillScore
    from prediff_amd.spectrum import SEVIRSpectralScore
    return {c.__name__: c for c in (SEVIRSkillScore, SEVIREnsembleScore, SEVIRFrameScore, SEVIRSpectralScore)}[name]


def fill(m):
    """A hand-made state, as after updates: every element different, the counts positive."""
    m._alloc_state("cpu")
    for i, t in enumerate(m._state_tensors()):
        t += (torch.arange(t.numel(), dtype=torch.float64).view(t.shape) * (i + 2) + 1).to(t.dtype)
    if hasattr(m, "num_members"):
        m.num_members = 4


def plain(x):
    """A compute() result as nested dicts / lists of Python numbers (NaN as a string, so that == compares it)."""
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    a = np.asarray(x, dtype=np.float64)
    return [repr(v) for v in a.reshape(-1).tolist()], a.shape


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, q):
    """Rank 0 holds a state, rank 1 made no update; both call sync() of each class in turn."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        for name in CLASSES:
            m = score_class(name)(layout="NTHWC", mode="1", seq_len=3)
            if name == "SEVIRSpectralScore":
                m.hw = HW
            if rank == 0:
                fill(m)
            m.sync()
            out[name] = ([t.numpy().copy() for t in m._state_tensors()], getattr(m, "num_members", None), plain(m.compute()))
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def synced():
    """{rank: {class name: (state arrays, num_members, compute())}} after one sync() per class over two gloo ranks."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("name", CLASSES)
def test_sync_with_an_idle_rank(synced, name):
    """sync() is a collective on every rank: the rank without updates takes part with a zero state, so both end with rank 0's numbers.
    (SEVIRSkillScore used to return early on such a rank and leave its peer in the all-reduce.)"""
    want = score_class(name)(layout="NTHWC", mode="1", seq_len=3)
    if name == "SEVIRSpectralScore":
        want.hw = HW
    fill(want)
    (s0, m0, c0), (s1, m1, c1) = synced[0][name], synced[1][name]
    assert len(s0) == len(s1) == len(want.STATE)
    for a, b, w in zip(s0, s1, want._state_tensors()):
        assert a.dtype == b.dtype and np.array_equal(a, w.numpy()) and np.array_equal(b, a)
    assert m0 == m1 == (4 if name == "SEVIREnsembleScore" else None)
    assert c0 == c1 == plain(want.compute())


def test_spectral_sync_needs_the_frame_sides():
    from prediff_amd.spectrum import SEVIRSpectralScore
    m = SEVIRSpectralScore(mode="1", seq_len=3)
    with pytest.raises(ValueError, match="hw"):
        m._alloc_state("cpu")                     # what sync() does on a rank without updates
    m.hw = HW
    m._alloc_state("cpu")
    assert m.sums.shape == (3, 3, 7) and m.frames.shape == (3,) and m.cells.shape == (7,)


@pytest.mark.parametrize("name", CLASSES)
def test_constructor_contract(name):
    cls = score_class(name)
    with pytest.raises(NotImplementedError):
        cls(layout="NTHWC", mode="3")
    if name in LAYOUT_CHECKED:
        with pytest.raises(ValueError):
            cls(layout="NTHWX")
        with pytest.raises(ValueError):
            cls(layout="NTHWC", metrics_list=("no_such_metric",))
    with pytest.raises(SEQ_LEN_ERROR[name]):
        cls(layout="NTHWC", mode="1")
    m = cls(layout="NTHWC", mode="1", seq_len=3)
    assert m.keep_seq_len_dim and m.Tk == 3 and all(t is None for t in m._state_tensors())
    assert cls(layout="NTHWC").Tk == 1


@pytest.mark.parametrize("name", CLASSES)
def test_compute_on_a_fresh_instance(name):
    """Nothing accumulated: NaN (0 / 0) or zeros (the skill scores' eps), never an exception."""
    for mode in ("0", "1", "2"):
        ret = score_class(name)(layout="NTHWC", mode=mode, seq_len=3).compute()
        leaves = []

        def walk(x):
            if isinstance(x, dict):
                for v in x.values():
                    walk(v)
            else:
                leaves.append(np.asarray(x, dtype=np.float64))
        walk(ret)
        assert leaves
        for a in leaves:
            assert np.all(np.isnan(a) | (a == 0.0)), (name, mode, a)


@pytest.mark.parametrize("name", CLASSES)
def test_workspace_is_kept_grown_and_replaced(name):
    m = score_class(name)(layout="NTHWC")
    cpu = torch.device("cpu")
    a = m._workspace(16, torch.float64, cpu)
    assert a.numel() == 16 and a.dtype == torch.float64 and a.device == cpu and m._ws is a
    assert m._workspace(16, torch.float64, cpu) is a and m._workspace(3, torch.float64, torch.zeros(1).device) is a
    b = m._workspace(17, torch.float64, cpu)
    assert b is not a and b.numel() == 17 and m._ws is b
    m.reset()
    assert m._ws is None


def test_one_member_limit():
    import prediff_amd.score_base as SB
    assert SB.MAX_MEMBERS == 512
    big, tgt = torch.zeros(513, 1, 1, 11, 11, 1), torch.zeros(1, 1, 11, 11, 1)
    for name, call in (("SEVIREnsembleScore", "update"), ("SEVIRFrameScore", "update_members"), ("SEVIRSpectralScore", "update_members")):
        m = score_class(name)(layout="NTHWC", **({"data_range": 1.0} if name == "SEVIRFrameScore" else {}))
        with pytest.raises(ValueError, match="513"):
            getattr(m, call)(big, tgt)            # checked before any device is touched
        with pytest.raises(ValueError, match="target.shape"):
            getattr(m, call)(big[:2, :, :, :10], tgt)


def test_sevir_skill_still_exports_the_axes_helpers():
    from prediff_amd import score_base
    from prediff_amd.sevir_skill import AXES, axes_of, parse_preprocess
    assert AXES == "NTHWC" and axes_of is score_base.axes_of and parse_preprocess is score_base.parse_preprocess
    x = torch.zeros(2, 5, 7, 3)                   # N H W T
    assert axes_of("NHWT", x) == ([2, 3, 5, 7, 1], [105, 1, 21, 3, 0])
    assert axes_of("NHWT", x.unsqueeze(0), lead=1)[0] == [2, 3, 5, 7, 1]
    assert parse_preprocess("sevir", "NHWT") == 1 and parse_preprocess("sevir_pool4", "NTHWC") == 4
