"""Static skeleton of every instantiation of a kernel template in an assembly file (hipcc, the shipped flags, -S or -save-temps):
instructions, basic blocks, registers, scratch, the scalar / move / 64-bit-address instruction classes a launch skeleton is made
of, and what stands between kernel entry and the first LDS-DMA.
    python tools/chain_isa.py FILE.s [kernel name, default chain_gemm_kernel] [substring of the demangled template arguments]
    python tools/chain_isa.py chain.s
    python tools/chain_isa.py fused_stage.s fused_up_conv_kernel "<32, 1, 2, 2, 1, 32, 8, 3"
"""
import collections, re, subprocess, sys
s = open(sys.argv[1]).read()
kernel = sys.argv[2] if len(sys.argv) > 2 else "chain_gemm_kernel"
sub = sys.argv[3] if len(sys.argv) > 3 else ""
WATCH = ("v_mov_b32", "v_mov_b64", "s_mul_i32", "s_mul_hi_u32", "s_add_i32", "s_add_u32", "s_addc_u32", "v_lshl_add_u64", "v_mad_u64_u32",
         "v_ashrrev_i32", "s_and_saveexec_b64", "s_cbranch", "s_nop", "s_load", "s_waitcnt")
print(f"{'kernel':78s} {'inst':>5s} {'bb':>4s} {'SALU':>5s} {'VALU':>5s} {'VGPR':>4s} {'SGPR':>4s} {'scr B':>5s} " +
      " ".join(f"{w.replace('_b32', '').replace('_i32', ''):>8s}"[-8:] for w in WATCH) + "  before the first LDS-DMA")
for m in re.finditer(r"^(_Z\w*%s\w*):\s*; @" % re.escape(kernel), s, re.M):
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.sub(r".*%s" % re.escape(kernel), "", name).split("(")[0]
    name = name.replace("(bool)0", "0").replace("(bool)1", "1").replace("false", "0").replace("true", "1")
    if sub not in name:
        continue
    end = s.index(".Lfunc_end", m.start())
    body = s[m.start():end].split("\n")
    tail = s[end:end + 4000]                       # the resource comment block behind the function
    res = lambda key: (re.search(r";\s*%s:\s*(\d+)" % key, tail) or [None, "?"])[1]      # noqa: E731
    ins = [ln.strip() for ln in body if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
    ops = collections.Counter(i.split()[0] for i in ins)
    blocks = 1 + sum(1 for ln in body if re.match(r"^\.LBB\d+_\d+:", ln))
    grp = lambda p, ex=(): sum(v for k, v in ops.items() if k.startswith(p) and not k.startswith(ex))   # noqa: E731
    first = next((i for i, x in enumerate(ins) if x.startswith("global_load_lds")), len(ins))
    waits = [x for x in ins[:first] if x.startswith("s_waitcnt")]
    full = [w for w in waits if "vmcnt(0)" in w]
    print(f"{name:78s} {len(ins):5d} {blocks:4d} {grp('s_'):5d} {grp('v_', ('v_mfma',)):5d} {res('NumVgprs'):>4s} {res('NumSgprs'):>4s} "
          f"{res('ScratchSize'):>5s} " + " ".join(f"{sum(v for k, v in ops.items() if k.startswith(w)):8d}" for w in WATCH) +
          f"  {first} inst, {len(waits)} s_waitcnt ({len(full)} with vmcnt(0))")
