"""p3v_kv_copy (the prompt prefix cache's device path) against torch slicing, BIT-equal.

Caches are filled with a position-coded pattern, destinations with a canary; after the launch the WHOLE destination
tensors are compared with a torch-sliced expectation, so every byte outside the destination runs is checked too.
Covered: element size 2 (bf16) and 1 (int8 codes + fp32 scale rows); hd 96 and 64; n_tok in {1, 7, 8, 9, 63, 64, 65,
2512, 2533}; every (src_t0, dst_t0) phase pair mod 8 (bf16) / mod 16 (int8); T strides of a real state (an odd number of
128-key tiles) and of a compact entry (tokens rounded up to 8); 4 jobs per launch with different phases; argument errors."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NL, NKV = 2, 2
N_TOK = [1, 7, 8, 9, 63, 64, 65, 2512, 2533]


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def odd_tiles(t):
    """Column stride of a real cache state (model.CacheState): whole 128-key tiles, an odd number of them."""
    tp = (t + 127) // 128 * 128
    return tp + 128 if (tp // 128) % 2 == 0 else tp


def coded(shape, es, salt, dev):
    """Every element names its own flat position (never a NaN pattern issue: compared as integers)."""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, device=dev, dtype=torch.int64) + salt
    if es == 2:
        return (idx % 65521).to(torch.int32).to(torch.int16).view(torch.bfloat16).view(shape)
    return (idx % 251).to(torch.uint8).view(shape)


def make_cache(B, T, hd, es, salt, dev, canary=False):
    """(k, vt) bf16 or (k8, v8t, ks, vs)."""
    if canary:
        if es == 2:
            k = torch.full((NL, B, NKV, T, hd), 0x7A5A, dtype=torch.int16, device=dev).view(torch.bfloat16)
            v = torch.full((NL, B, NKV, hd, T), 0x7B5B, dtype=torch.int16, device=dev).view(torch.bfloat16)
            return (k, v)
        return (torch.full((NL, B, NKV, T, hd), 0xA5, dtype=torch.uint8, device=dev), torch.full((NL, B, NKV, hd, T), 0xB5, dtype=torch.uint8, device=dev),
                torch.full((NL, B, NKV, T), -7.0, dtype=torch.float32, device=dev), torch.full((NL, B, NKV, T), -9.0, dtype=torch.float32, device=dev))
    kv = (coded((NL, B, NKV, T, hd), es, salt, dev), coded((NL, B, NKV, hd, T), es, salt + 17, dev))
    if es == 1:
        kv += (torch.arange(NL * B * NKV * T, device=dev, dtype=torch.float32).view(NL, B, NKV, T) + 0.5,
               -torch.arange(NL * B * NKV * T, device=dev, dtype=torch.float32).view(NL, B, NKV, T) - 0.25)
    return kv


def expect(dst, src, b_s, t0_s, b_d, t0_d, n):
    """The same move with torch slicing, on clones."""
    dst[0][:, b_d, :, t0_d:t0_d + n, :] = src[0][:, b_s, :, t0_s:t0_s + n, :]
    dst[1][:, b_d, :, :, t0_d:t0_d + n] = src[1][:, b_s, :, :, t0_s:t0_s + n]
    for d, s in zip(dst[2:], src[2:]):
        d[:, b_d, :, t0_d:t0_d + n] = s[:, b_s, :, t0_s:t0_s + n]


def same(a, b):
    return all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("n", N_TOK)
@pytest.mark.parametrize("hd", [96, 64])
@pytest.mark.parametrize("es", [2, 1])
def test_every_phase_pair_bit_equal_and_nothing_else_written(ops, es, hd, n):
    dev = "cuda:0"
    ph = 16 // es                                               # phases of a 16-byte store: 8 bf16 / 16 int8 elements
    state_T = odd_tiles(n + 2 * ph + 40)
    entry_T = (n + ph + 7) // 8 * 8 + 8                         # a compact entry (+ room for the source phase)
    assert (state_T // 128) % 2 == 1
    slot = make_cache(3, state_T, hd, es, 3, dev)               # "slot state": 3 rows
    entry = make_cache(1, entry_T, hd, es, 1001, dev)           # "store entry": one row
    pairs = [(s0, d0) for s0 in range(ph) for d0 in range(ph)]
    for c in range(0, len(pairs), 4):
        chunk = pairs[c:c + 4]
        # restore-shaped: entry -> 4 rows of a fresh slot state, each job its own phases (odd ones included: pad = column - S)
        dst = make_cache(4, state_T, hd, es, 0, dev, canary=True)
        want = tuple(t.clone() for t in dst)
        jobs = []
        for row, (s0, d0) in enumerate(chunk):
            jobs.append((entry, 0, s0, dst, row, 25 + d0, n))
            expect(want, entry, 0, s0, row, 25 + d0, n)
        ops.kv_copy(jobs)
        assert same(dst, want), (es, hd, n, chunk, "entry -> slot")
        # capture-shaped: rows of the slot state -> 4 rows of a compact tensor
        dst = make_cache(4, entry_T, hd, es, 0, dev, canary=True)
        want = tuple(t.clone() for t in dst)
        jobs = []
        for row, (s0, d0) in enumerate(chunk):
            jobs.append((slot, row % 3, 9 + s0, dst, row, d0, n))
            expect(want, slot, row % 3, 9 + s0, row, d0, n)
        ops.kv_copy(jobs)
        assert same(dst, want), (es, hd, n, chunk, "slot -> entry")
    torch.cuda.synchronize()


def test_same_tensor_other_row_and_empty_job(ops):
    """Row to row inside ONE state is legal (disjoint rows), and an n_tok = 0 job writes nothing."""
    dev = "cuda:0"
    st = make_cache(3, 384, 96, 2, 5, dev)
    want = tuple(t.clone() for t in st)
    expect(want, st, 0, 3, 2, 10, 100)
    ops.kv_copy([(st, 0, 3, st, 2, 10, 100), (st, 0, 0, st, 1, 0, 0)])
    assert same(st, want)


def _job(L, src, dst, **kw):
    j = L.KvCopyJob()
    j.k_src, j.v_src, j.k_dst, j.v_dst = src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
    if len(src) == 4:
        j.ks_src, j.vs_src, j.ks_dst, j.vs_dst = src[2].data_ptr(), src[3].data_ptr(), dst[2].data_ptr(), dst[3].data_ptr()
    j.B_src, j.T_src, j.B_dst, j.T_dst = src[0].shape[1], src[0].shape[3], dst[0].shape[1], dst[0].shape[3]
    j.b_src = j.b_dst = j.t0_src = j.t0_dst = 0
    j.n_tok = 8
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def test_argument_errors_return_err_arg_and_launch_nothing(ops):
    L = ops.L
    lib, dev = L.lib(), "cuda:0"
    src, dst = make_cache(2, 128, 96, 2, 1, dev), make_cache(2, 128, 96, 2, 0, dev, canary=True)
    want = tuple(t.clone() for t in dst)
    stream = torch.cuda.current_stream().cuda_stream

    def call(jobs, n_jobs=None, nl=NL, nkv=NKV, hd=96, es=2):
        arr = (L.KvCopyJob * max(len(jobs), 1))(*jobs)
        return lib.p3v_kv_copy(arr, len(jobs) if n_jobs is None else n_jobs, nl, nkv, hd, es, stream)

    ok = _job(L, src, dst)
    bad = [
        call([ok], n_jobs=0), call([ok] * 5), call([ok], es=4), call([ok], es=3), call([ok], nl=0), call([ok], hd=0),
        call([ok], hd=100),                                       # 200-byte K rows: not 16-byte multiples
        call([_job(L, src, dst, b_src=2)]), call([_job(L, src, dst, b_dst=-1)]),
        call([_job(L, src, dst, t0_src=121)]),                    # the run leaves its row: 121 + 8 > 128
        call([_job(L, src, dst, t0_dst=124)]), call([_job(L, src, dst, t0_dst=-1)]), call([_job(L, src, dst, n_tok=-1)]),
        call([_job(L, src, dst, n_tok=129)]),
        call([_job(L, src, dst, k_src=0)]), call([_job(L, src, dst, v_dst=0)]),
        call([_job(L, src, dst, k_dst=dst[0].data_ptr() + 2)]),   # K base not 16-byte aligned
        call([_job(L, src, dst, v_src=src[1].data_ptr() + 1)]),   # bf16 V base at an odd byte
        call([_job(L, src, dst, ks_src=src[0].data_ptr())]),      # one scale pointer of four
        call([_job(L, src, src, t0_dst=4)]),                      # overlapping source and destination (same row, tokens 0..8 / 4..12)
        call([_job(L, src, dst, b_dst=1, t0_dst=0), _job(L, src, dst, b_dst=1, t0_dst=7)]),     # two jobs, overlapping destinations
        call([_job(L, src, dst), _job(L, dst, src, b_src=0, b_dst=1)]),                          # job 1 reads what job 0 writes
        lib.p3v_kv_copy(None, 1, NL, NKV, 96, 2, stream),
    ]
    assert bad == [-22] * len(bad), bad
    # a view into the destination's allocation as source: refused outright
    assert call([_job(L, (dst[0][1:], dst[1][1:]), dst, B_src=2, T_src=128)]) == -22
    torch.cuda.synchronize()
    assert same(dst, want)
    assert call([ok]) == 0 and call([_job(L, src, src, b_dst=1)]) == 0       # the legal neighbours of the cases above
    with pytest.raises(ValueError):
        ops.kv_copy([])
    with pytest.raises(ValueError):
        ops.kv_copy([(src, 0, 0, dst, 0, 0, 1)] * 5)
    with pytest.raises((TypeError, ValueError)):
        ops.kv_copy([(src, 0, 0, make_cache(2, 128, 96, 1, 0, dev), 0, 0, 1)])
    assert isinstance(ctypes.sizeof(L.KvCopyJob), int) and ctypes.sizeof(L.KvCopyJob) == 104
