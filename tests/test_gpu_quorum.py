"""GPU parity of the quorum commit-index kernel and the session expiry sweep vs the oracle (bit-exact)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda().view(torch.uint64)


def _h(t):
    import torch

    return t.view(torch.int64).cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("groups,replicas", [(1, 5), (2, 5), (1001, 5), (1 << 20, 5), (4096, 3), (4097, 7), (999, 4), (64, 1)])
def test_quorum_parity(groups, replicas):
    import torch

    from copycat_amd.engine import quorum_commit
    from copycat_amd.workload import quorum_groups
    from oracle.oracle_py import quorum_commit as oq

    match, ts, ci = quorum_groups(groups, replicas=replicas, seed=groups + replicas)
    out = torch.zeros(groups, dtype=torch.int64, device="cuda")
    quorum_commit(_t(match), _t(ts), _t(ci), out)
    torch.cuda.synchronize()
    assert np.array_equal(_h(out), oq(match, ts, ci))


def _off8(a):
    """the array on the device, starting 8 bytes into its tensor (8-byte but not 16-byte aligned)"""
    import torch

    a = np.ascontiguousarray(a)
    t = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda")
    t[1:] = torch.from_numpy(a.reshape(-1).view(np.int64)).cuda()
    out = t[1:].view(torch.uint64).view(a.shape)
    assert out.data_ptr() % 16 == 8
    return out


def _edge_case(groups, replicas, misalign=None):
    """cc_quorum_commit on abi_cases.quorum_edge_groups against the oracle; the output is prefilled with a value no
    group can produce from these inputs (0x5A...), so a group no thread wrote fails too.  misalign: the pointer that
    starts 8 bytes into its tensor."""
    import torch

    from copycat_amd.engine import quorum_commit
    from oracle.oracle_py import quorum_commit as oq
    from tests.abi_cases import quorum_edge_groups

    match, ts, ci = quorum_edge_groups(groups, replicas, seed=groups * 31 + replicas)
    want = oq(match, ts, ci)
    share = float((want != ci).mean())
    assert 0.05 < share < 0.5, share  # (the reference alone: 0.15 .. 0.29)
    fill = np.full(groups, 0x5A5A5A5A5A5A5A5A, np.uint64)
    up = {name: (_off8 if misalign == name else _t)(arr) for name, arr in
          (("match", match), ("ts", ts), ("ci", ci), ("out", fill))}
    quorum_commit(up["match"], up["ts"], up["ci"], up["out"])
    torch.cuda.synchronize()
    got = _h(up["out"])
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("groups,replicas", [((1 << 20) + 1538, 3), ((1 << 20) + 1538, 5), ((1 << 20) + 1538, 7),
                                             (524_288 + 257, 4), (524_288 + 257, 5)])
def test_quorum_grid_stride_loops(groups, replicas):
    """More groups than one pass of the grid holds: 2,048 x 256 pairs in k_quorum<R> (even groups, aligned), 2,048 x
    256 groups in k_quorum_generic (odd groups)."""
    _edge_case(groups, replicas)


@pytest.mark.parametrize("replicas", [1, 2, 3, 4, 5, 6, 7, 8, 15, 16])
@pytest.mark.parametrize("groups", [4098, 4097])
def test_quorum_replica_counts_over_the_unsigned_range(groups, replicas):
    """Every dispatch (k_quorum<3 / 5 / 7> for even groups, k_quorum_generic for the rest) on inputs at 0, 2^63 and
    2^64 - 1 with ties: a signed comparison or a wrong rank fails."""
    _edge_case(groups, replicas)


@pytest.mark.parametrize("misalign", ["match", "ts", "ci", "out"])
@pytest.mark.parametrize("replicas", [3, 5, 7])
def test_quorum_misaligned_pointers_take_the_generic_kernel(misalign, replicas):
    """An even `groups` with one pointer 8 bytes off 16-byte alignment: the same answers (the 16-byte loads of
    k_quorum<R> would need the alignment)."""
    _edge_case(4098, replicas, misalign)


def test_quorum_refusals_leave_the_output_untouched():
    import torch

    from copycat_amd import abi
    from copycat_amd.engine import lib
    from tests.abi_cases import quorum_edge_groups

    groups = 1024
    match, ts, ci = quorum_edge_groups(groups, 16, seed=5)
    pad = np.zeros((1, groups), np.uint64)
    m, t, c = _t(np.concatenate([match, pad])), _t(ts), _t(ci)
    out = torch.full((groups,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    L = lib()
    p = lambda x: x.data_ptr()  # noqa: E731
    for replicas in (0, 17):
        assert L.cc_quorum_commit(p(m), replicas, groups, p(t), p(c), p(out), None) == abi.CC_ERR_INVALID
    for null in range(4):
        args = [p(m), p(t), p(c), p(out)]
        args[null] = None
        assert L.cc_quorum_commit(args[0], 5, groups, args[1], args[2], args[3], None) == abi.CC_ERR_INVALID
    assert L.cc_quorum_commit(p(m), 5, 0, p(t), p(c), p(out), None) == abi.CC_OK  # no group: nothing to do
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("now", [10_000_000, (1 << 63) + 5, 3])
@pytest.mark.parametrize("timeout", [0, 5000, (1 << 63) - 1, 1 << 63, (1 << 64) - 1])
def test_expiry_over_the_unsigned_range(now, timeout):
    """Timeouts at and past 2^63 (the kernel takes the timeout as a signed 64-bit value, as the oracle does), stamps
    with the top bit set, in the future and at the signed boundary of now - last; 1,001 sessions: a ragged last word
    and a last lane pair with one session."""
    import torch

    from copycat_amd.engine import expire_sweep
    from oracle.oracle_py import expire_sweep as oe
    from tests.abi_cases import expiry_edge_sessions

    sessions = 1001
    last = expiry_edge_sessions(sessions, now, seed=now % 1000 + 1)
    bm = torch.zeros((sessions + 63) // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    expire_sweep(_t(last), now, timeout, bm, cnt)
    torch.cuda.synchronize()
    ebm, ec = oe(last, now, timeout)
    assert np.array_equal(_h(bm), ebm)
    assert int(_h(cnt)[0]) == ec
    if timeout == 5000:
        assert 0 < ec < sessions


def test_expiry_refusals():
    """No session is CC_OK and touches nothing; a d_last 8 bytes off 16-byte alignment is refused (the kernel loads two
    stamps per lane)."""
    import torch

    from copycat_amd import abi
    from copycat_amd.engine import lib

    last = np.arange(1, 257, dtype=np.uint64)
    bm = torch.full((4,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    L = lib()
    d = _t(last)
    assert L.cc_expire_sweep(d.data_ptr(), 0, 1000, 10, bm.data_ptr(), cnt.data_ptr(), None) == abi.CC_OK
    off = _off8(last)
    assert L.cc_expire_sweep(off.data_ptr(), 256, 1000, 10, bm.data_ptr(), cnt.data_ptr(), None) == abi.CC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((bm == 0x5A5A5A5A).all()) and int(cnt[0]) == 77


@pytest.mark.parametrize("sessions", [1, 63, 64, 127, 128, 129, 100_000, 1 << 20])
def test_expiry_parity(sessions):
    import torch

    from copycat_amd.engine import expire_sweep
    from copycat_amd.workload import expiry_sessions
    from oracle.oracle_py import expire_sweep as oe

    last, now, timeout = expiry_sessions(sessions, seed=sessions)
    last[: min(3, sessions)] = now + 5  # keep-alive stamped in the future never expires
    words = (sessions + 63) // 64
    bm = torch.zeros(words, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    expire_sweep(_t(last), now, timeout, bm, cnt)
    torch.cuda.synchronize()
    ebm, ec = oe(last, now, timeout)
    assert np.array_equal(_h(bm), ebm)
    assert int(_h(cnt)[0]) == ec
