"""Static skeleton of every chain_gemm_kernel instantiation in an assembly file of csrc/chain.hip (hipcc, the shipped flags, -S):
instructions, basic blocks, the scalar / move / 64-bit-address instructions the launch skeleton is made of, and what stands between
kernel entry and the first LDS-DMA.
    python tools/chain_isa.py chain.s [substring of the demangled name]"""
import collections, re, subprocess, sys
s = open(sys.argv[1]).read()
sub = sys.argv[2] if len(sys.argv) > 2 else ""
WATCH = ("v_mov_b32", "s_mul_i32", "s_mul_hi_u32", "s_add_i32", "s_add_u32", "s_addc_u32", "v_lshl_add_u64", "v_mad_u64_u32",
         "s_and_saveexec_b64", "s_cbranch_execz", "s_nop", "s_load")
print(f"{'kernel':58s} {'inst':>5s} {'bb':>4s} {'SALU':>5s} {'VALU':>5s} " + " ".join(f"{w.replace('_b32', '').replace('_b64', ''):>8s}"[-8:] for w in WATCH) +
      "  before the first LDS-DMA")
for m in re.finditer(r"^(_Z\w*chain_gemm_kernel\w*):\s*; @", s, re.M):
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.sub(r".*chain_gemm_kernel", "", name).split("(")[0]
    if sub not in name:
        continue
    body = s[m.start():s.index(".Lfunc_end", m.start())].split("\n")
    ins = [ln.strip() for ln in body if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
    ops = collections.Counter(i.split()[0] for i in ins)
    blocks = 1 + sum(1 for ln in body if re.match(r"^\.LBB\d+_\d+:", ln))
    grp = lambda p, ex=(): sum(v for k, v in ops.items() if k.startswith(p) and not k.startswith(ex))   # noqa: E731
    first = next((i for i, x in enumerate(ins) if x.startswith("global_load_lds")), len(ins))
    waits = [x for x in ins[:first] if x.startswith("s_waitcnt")]
    full = [w for w in waits if "vmcnt(0)" in w]
    print(f"{name:58s} {len(ins):5d} {blocks:4d} {grp('s_'):5d} {grp('v_', ('v_mfma',)):5d} " +
          " ".join(f"{sum(v for k, v in ops.items() if k.startswith(w)):8d}" for w in WATCH) +
          f"  {first} inst, {len(waits)} s_waitcnt ({len(full)} with vmcnt(0))")
