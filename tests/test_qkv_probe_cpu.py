"""The probes of tests/qkv_probe.py, checked on the references alone (no GPU).  Three things:
  * the conditions the rules lean on hold for every case of both families: proj_probe's own (exact sums, >= 1 % rounding ties and
    >= 50 % sums that are no bf16 value on GRID: asserted by its builder), and the judged brackets of Q, K and V^T ONE value on >= 98 %
    of the elements;
  * a plain torch-fp32 restatement of the documented arithmetic -- fp32 sums, the bias, one rounding, RopeProbe's fp32 rotation with
    q_scale before the one rounding, every token stored at its own (b, l) -- passes every rule on every case;
  * every planted defect, applied to that restatement, fails on EVERY case on which it exists:
      pair_half32         the rotation partner taken 32 columns away instead of hd / 2 (a block of 16 pairs straddles a head at hd = 96)
      pos_dpos0           rotation position dpos0 + l instead of past + l
      tab_div_ignored     table row b instead of b / tab_div
      scale_keys          q_scale applied to the keys as well
      scale_after         q_scale applied after the rounding
      bias_half           the second halves of the pairs get the first halves' bias
      v_bias_by_token     the V bias indexed by token
      m_base_dropped      the small-tile launch behind the big tiles takes its own row 0 for token 0
      k_head_stride_nh    the K head index strided by nh instead of nkv
      v_odd_shift         a V^T run at an odd offset shifted by one token
      v_wrap_once         a V^T run that crosses a batch-row end wraps once, whatever the row length
      v_tail_dropped      the last M mod 8 tokens of V not stored
      clamped_row_stored  row M (a clamped row of the last tile) stored
      drop_last_ktile     the last K-tile left out of the sums
      lda_as_k            A read with lda taken as K
A kernel with such a defect therefore cannot pass tests/test_qkv_kernels_gpu.py.  The route of every case is asserted here too: with a
CU count given p3v_gemm_route asks no device."""
import pytest

import qkv_probe as qp

ids = lambda c: c.id
CUS = 256


def test_table_reaches_every_path():
    cs = qp.CASES
    by = lambda k: [c for c in cs if c.kernel == k]
    assert {c.kernel for c in cs} == {qp.SKINNY, qp.K128, qp.K256, qp.K256 + "+" + qp.K128}
    assert {(c.hd, c.nh, c.nkv) for c in by(qp.SKINNY)} == {(96, 2, 4), (64, 2, 2), (32, 4, 4), (128, 1, 1)}
    assert {(c.B, c.L) for c in by(qp.SKINNY)} == {(1, 9), (1, 129), (2, 64), (3, 85), (4, 61), (16, 1), (3, 3), (5, 5), (6, 7)}
    assert {64, 192, 3072} == {c.K for c in by(qp.SKINNY)} and sum(c.K == 3072 for c in by(qp.SKINNY)) >= 2
    assert not any(c.bias for c in by(qp.SKINNY)) and all(9 <= c.M <= 256 for c in by(qp.SKINNY))
    assert {1024, 1025, 1029} <= {c.M for c in by(qp.K128)} and {(96, 4, 4), (96, 8, 4), (64, 2, 2)} <= {(c.hd, c.nh, c.nkv) for c in by(qp.K128)}
    assert any(c.bias and c.null and not c.off_is_past and (c.B, c.L, c.K) == (2, 577, 1024) for c in by(qp.K128))
    assert {(c.hd, c.nh, c.nkv) for c in cs if c.rows_big} == {(96, 8, 8), (64, 4, 4)}
    assert {(c.B, c.L) for c in by(qp.K256 + "+" + qp.K128)} == {(2, 550), (3, 343)} and any(c.big_rows == qp.AUTO for c in cs)
    for k in (qp.SKINNY, qp.K128, qp.K256):                                # every kernel: K = 3072, strides, a rotation at some offset
        assert any(c.K == 3072 for c in by(k)) and any(c.ld for c in by(k)) and any(c.past and not c.null for c in by(k)), k
    assert any(c.bias and not c.null for c in cs)
    assert {0, 8, 64, 200} <= {c.past for c in cs} and any(c.past == 13 and not c.off_is_past for c in cs)
    assert any(c.tab_div == 3 and c.B == 6 for c in cs) and {True, False} == {c.prescale for c in cs}
    assert all(c.dst_t % 8 == 0 for c in cs) and any(c.dst_t % 64 for c in cs)
    for d, exists in qp.DEFECTS.items():                                   # every defect exists on some case, the short rows on the short rows
        assert any(exists(c) for c in cs), d
    assert {(c.B, c.L) for c in cs if qp.DEFECTS["v_wrap_once"](c)} == {(16, 1), (3, 3), (5, 5)}


@pytest.mark.parametrize("case", qp.CASES, ids=ids)
def test_route(case):
    from phi_3_vision_mlx_amd import ops
    old = [(name, ops.set_tuning(name, value)) for name, value in case.knobs]
    try:
        qp.check_route(ops, case, cu_count=CUS)
    finally:
        for name, value in reversed(old):
            ops.set_tuning(name, value)


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.CASES, ids=ids)
def test_reference_passes_and_every_defect_fails(case, family):
    pr = qp.probe(case, family)                                            # (proj_probe's builder assertions run here)
    shares = pr.unique_shares()
    line = f"{case.id} [{family}]: bracket is one value on " + ", ".join(f"{n} {100 * s:.2f} %" for n, s in shares.items())
    if pr.grid:
        line += f"; {100 * pr.lin.ties:.1f} % ties, {100 * pr.lin.unrep:.0f} % sums that are no bf16 value"
    print(line)
    assert min(shares.values()) >= qp.MIN_UNIQUE
    msg = pr.verify(pr.emulate())
    assert msg == "", f"the clean restatement: {msg}"
    for defect, exists in qp.DEFECTS.items():
        if exists(case):
            msg = pr.verify(pr.emulate(defect))
            print(f"  {defect}: {msg}")
            assert msg != "", f"{defect} goes unseen on {case.id} [{family}]"
