"""Static look at the streaming GEMV kernels (k_gemv3*) in `hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` output.

  python tools/gemv_isa.py table p3v_gemv_b13.s            the columns of profiles/pack13_gemv_isa.txt
  python tools/gemv_isa.py hash old.s new.s [old2.s new2.s ...]
                                                           sha256 of every k_gemv3* kernel's text with comments and label numbers
                                                           removed, in both builds (profiles/gemv_stream_isa_unchanged.txt)
No GPU needed."""
import hashlib
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    """{mangled name: (instruction lines, vgpr count, scratch bytes)} of the k_gemv3* kernels of one -S file"""
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        v = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2))
        if v and p:
            meta[m.group(1)] = (int(v.group(1)), int(p.group(1)))
    out = {}
    for m in re.finditer(r"^(_Z\d+k_gemv3\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = [re.sub(r"\s*;.*", "", l).strip() for l in m.group(2).split("\n")]
        out[m.group(1)] = ([l for l in lines if l], *meta[m.group(1)])
    return out


def normalised(lines):
    t = "\n".join(l for l in lines if not l.startswith((".loc", ".file", ".cfi", ".p2align")))
    return re.sub(r"\.L(BB|tmp|func_end|func_begin)[0-9_]+", r".L\1", t)


def table(path):
    ks = kernels(path)
    names = demangle(list(ks))
    print("MT,NST,CH[,STEP] |  vgpr waves  scr scratch-instr gload   x4   x3   x2 dot2 perm pk_min pk_mad  vm0  vmN")
    for k in sorted(ks, key=lambda n: names[n]):
        ins, vgpr, scr = ks[k]
        cnt = lambda pat: sum(1 for l in ins if re.match(pat, l))
        vm = [int(m.group(1)) for l in ins for m in [re.match(r"s_waitcnt.*vmcnt\((\d+)\)", l)] if m]
        waves = min(8, 512 // (-(-vgpr // 8) * 8))
        # "1,1,6" of k_gemv3<GemvBf16, 1, 1, 6>; a policy that is a template itself (GemvB13<true>) puts its argument in front: "true 1,1,6"
        m = re.match(r".*?<\w+(?:<(\w+)>)?, ([^>]*)>", names[k])
        short = ((m.group(1) + " ") if m.group(1) else "") + m.group(2).replace(" ", "")
        print("%-16s | %5d %5d %4d %13d %5d %4d %4d %4d %4d %4d %6d %6d %4d %4d" % (
            short, vgpr, waves, scr, cnt("scratch_"), cnt("global_load"), cnt("global_load_dwordx4"), cnt("global_load_dwordx3"),
            cnt("global_load_dwordx2"), cnt("v_dot2c"), cnt("v_perm_b32"), cnt("v_pk_min_u16"), cnt("v_pk_mad_u16"),
            sum(1 for v in vm if v == 0), sum(1 for v in vm if v > 0)))
    print("%d kernels" % len(ks))


def hashes(pairs):
    same = True
    for old, new in pairs:
        a, b = kernels(old), kernels(new)
        names = demangle(sorted(set(a) | set(b)))
        assert names, "no k_gemv3* kernel in " + old
        print("%s -> %s" % (old, new))
        for k in sorted(names, key=lambda n: names[n]):
            ha = hashlib.sha256(normalised(a[k][0]).encode()).hexdigest() if k in a else "-" * 64
            hb = hashlib.sha256(normalised(b[k][0]).encode()).hexdigest() if k in b else "-" * 64
            same &= ha == hb
            print("  %-9s %s  %s  %s" % ("identical" if ha == hb else "DIFFERENT", ha, hb, re.sub(r"void |\(.*", "", names[k])))
    print("all identical" if same else "DIFFERENCES FOUND")
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "table":
        table(sys.argv[2])
    else:
        sys.exit(hashes(list(zip(sys.argv[2::2], sys.argv[3::2]))))
