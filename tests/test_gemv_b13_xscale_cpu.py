"""The identity behind the scaled decode of the 13-bit packed GEMV (GemvB13<true> in p3v_gemv_b13.hip), in torch on
the host: a weight's code s | q5 | m7, read as bf16, is the weight times 2^-(base - 1); with the activations times 2^(base - 1) every
product is the same fp32 number, so every sum taken in the same order has the same bits.  No GPU."""
import pytest
import torch

BF16, F32, I16, I32 = torch.bfloat16, torch.float32, torch.int16, torch.int32
MAX_SHIFT = 96                               # the launcher's rule: scaled decode for base - 1 <= 96 (every |x| < 2^32 fits)


def bits(t):
    return t.view(I16).to(I32) & 0xffff


def from_bits(b):
    return b.to(I16).view(BF16)              # (0x8000.. wraps onto the sign)


def codes(w):
    """(w' = the codes of w read as bf16, shift = base - 1) as the pack kernel chooses them: base = max(1, largest exponent - 30)."""
    b = bits(w)
    e, m, s = (b >> 7) & 0xff, b & 0x7f, b & 0x8000
    assert not ((e == 255) | ((e == 0) & (m != 0))).any()                 # no Inf / NaN / denormal weight
    base = max(1, int(e.max()) - 30)
    assert int(e[e != 0].min()) >= base                                   # the matrix fits the window
    q = torch.where(e == 0, torch.zeros_like(e), e - base + 1)
    assert int(q.max()) <= 31
    return from_bits(s | (q << 7) | m), base - 1


def window_matrix(e_top, rows, K, seed):
    """every pattern of the format under largest exponent e_top (31 binades x 128 mantissas x both signs, +0 and -0), shuffled, repeated"""
    e, m = torch.arange(e_top - 30, e_top + 1, dtype=I32), torch.arange(128, dtype=I32)
    mag = ((e[:, None] << 7) | m[None, :]).reshape(-1)
    pats = torch.cat([mag, mag | 0x8000, torch.tensor([0x0000, 0x8000], dtype=I32)])
    assert rows * K >= pats.numel()
    perm = torch.randperm(pats.numel(), generator=torch.Generator().manual_seed(seed))
    return from_bits(pats[perm].repeat(-(-rows * K // pats.numel()))[:rows * K]).reshape(rows, K).contiguous()


def normal_matrix(rows, K, seed):
    w = (torch.randn((rows, K), generator=torch.Generator().manual_seed(seed)) * 0.02).to(BF16)
    e = (bits(w) >> 7) & 0xff
    w[e < int(e.max()) - 30] = 0.0                                          # (what would make the pack refuse the matrix)
    w[0, 3], w[1, 5] = 0.0, -0.0                                            # planted zeros of both signs
    return w


def x_family(kind, K, shift, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(K, generator=gen).to(BF16)
    if kind == "zeros":
        x[torch.randperm(K, generator=gen)[:K // 8]] = 0.0
        x[1] = -0.0
    elif kind == "largest":                                                 # 2^(127 - shift) * 1.5 .. * 1.9921875: the last binade that fits
        mant = torch.randint(64, 128, (K,), generator=gen, dtype=I32)
        sign = torch.randint(0, 2, (K,), generator=gen, dtype=I32) << 15
        x = from_bits(sign | ((254 - shift) << 7) | mant)
    return x


CASES = [("window", 3072), ("window", 8192), ("normal", 3072), ("normal", 8192)]


@pytest.mark.parametrize("kind", ["normal", "zeros", "largest"])
@pytest.mark.parametrize("matrix,K", CASES)
def test_scaled_products_and_sums_are_the_exact_ones(matrix, K, kind):
    w = window_matrix(127, 4, K, 1) if matrix == "window" else normal_matrix(4, K, 2)
    wp, shift = codes(w)
    assert shift == MAX_SHIFT if matrix == "window" else 0 < shift < MAX_SHIFT
    scale = torch.tensor(2.0 ** shift, dtype=F32)
    assert torch.equal(bits((wp.float() * scale).to(BF16)), bits(w))        # w' * 2^shift == w, signs of the zeros included
    x = x_family(kind, K, shift, 3 + K)
    xp = (x.float() * scale).to(BF16)                                       # what the kernel stages
    assert torch.isfinite(xp.float()).all()
    assert torch.equal(xp.float(), x.float() * scale)                       # (a power of two: nothing is rounded)
    if kind == "largest":
        assert float(xp.float().abs().max()) == float(torch.finfo(BF16).max)
    a, b = w.float() * x.float()[None, :], wp.float() * xp.float()[None, :]
    finite = torch.isfinite(a)
    assert finite.all() or kind == "largest"                                # (|w| up to 2 times |x| up to 2^(128 - shift) may overflow: alike)
    assert torch.equal(a.view(I32), b.view(I32))                            # every product, bit for bit
    # sequential fp32 sums of the pairs a v_dot2c takes, lane order aside: acc += p[2i] + p[2i + 1]
    sa, sb = torch.zeros(4, dtype=F32), torch.zeros(4, dtype=F32)
    pa, pb = a[:, 0::2] + a[:, 1::2], b[:, 0::2] + b[:, 1::2]
    for i in range(0, K // 2, 64):                                          # (64 pairs a step: the order is still one fixed order)
        sa = sa + pa[:, i:i + 64].sum(dim=1)
        sb = sb + pb[:, i:i + 64].sum(dim=1)
    assert torch.equal(sa.view(I32), sb.view(I32))
    ca, cb = torch.cumsum(pa[:, :512], dim=1), torch.cumsum(pb[:, :512], dim=1)   # and strictly one after the other
    assert torch.equal(ca.view(I32), cb.view(I32))


def test_small_window_and_zero_shift():
    w = window_matrix(31, 4, 3072, 4)                                       # exponents 1 .. 31: base 1, the codes ARE the weights
    wp, shift = codes(w)
    assert shift == 0 and torch.equal(bits(wp), bits(w))
    w = window_matrix(100, 4, 3072, 5)
    wp, shift = codes(w)
    assert shift == 69 and torch.equal(bits((wp.float() * 2.0 ** 69).to(BF16)), bits(w))


def test_eligibility_rule_is_the_range_of_the_activations():
    """base - 1 <= 96 is exactly: every bf16 |x| < 2^32 keeps a finite scaled value; and for an eligible matrix the largest x that
    fits is 2^(127 - shift) * 1.9921875."""
    below_2_32 = from_bits(torch.tensor([((127 + 31) << 7) | 0x7f], dtype=I32)).float()     # 2^31 * 1.9921875
    table = []
    for base in range(1, 225):
        shift = base - 1
        fits = bool(torch.isfinite((below_2_32 * torch.tensor(2.0 ** shift, dtype=F32)).to(BF16).float()).all()) if shift < 128 else False
        table.append((base, fits))
        assert fits == (shift <= MAX_SHIFT), base
        if fits:
            top = from_bits(torch.tensor([((254 - shift) << 7) | 0x7f], dtype=I32)).float()
            nxt = from_bits(torch.tensor([((255 - shift) << 7) | 0x00], dtype=I32)).float()
            s = torch.tensor(2.0 ** shift, dtype=F32)
            assert torch.isfinite((top * s).to(BF16).float()).all() and not torch.isfinite((nxt * s).to(BF16).float()).any()
    assert [b for b, f in table if f] == list(range(1, 98))
    assert 127 - 30 - 1 == MAX_SHIFT                                        # the window under largest exponent 127 sits on the edge
