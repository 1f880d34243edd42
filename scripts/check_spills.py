"""(build container, no GPU) register spills of the persistent / two-source GEMM instantiations: compiles the GEMM family files
(csrc/koaf_gemm*.hip, with the Makefile's own flags) with -Rpass-analysis=kernel-resource-usage (1 min) and prints VGPRs / spilled VGPRs / scratch per instantiation that spills, against the
counts recorded when the round-4 regression was fixed (a 64-bit row index in the shared epilogue had cost every kernel ~30 VGPRs and
the persistent 1x1 kernels 40-90 spilled registers: +40 ms per step, invisible in the build output).
The one-pass optimizer / BCE kernels (koaf_optim.hip, koaf_bce.hip) and the kernels on the 256-row tile schedule of koaf_tile256.h
(koaf_wgrad1.hip, koaf_fwd_s2.hip, koaf_dgrad_s2.hip, koaf_fwd1.hip) are listed too and must not spill at all.
    python scripts/check_spills.py"""
import re, sys
from pathlib import Path
from compare_kernels import compile_commands, run_all
CS = Path(__file__).resolve().parent.parent / "oaprogressionmmf_amd" / "csrc"
RECORDED = {   # template arguments -> spilled VGPRs at the fixed build (koaf_gemm_kernel<BM, BN, AM, BMD, TFA, TFB, VEC, F16, NT, ACT, EMIT, SD>)
    "128,128,0,6,1,0,1,1,256,0,0,0": 7, "128,128,1,6,1,0,1,1,256,0,0,0": 35, "128,128,1,6,0,0,1,1,256,0,0,0": 14,
    "128,128,2,6,0,0,1,1,256,0,0,0": 15, "128,128,0,6,2,0,1,1,256,0,0,0": 0, "128,128,0,6,3,0,1,1,256,0,0,0": 0,
    "128,64,12,6,0,0,1,1,256,0,0,0": 0, "256,128,9,6,0,0,1,1,512,0,0,0": 0,
    # the streamed kernels (A mode 13): the persistent one-source ones carry two k-tiles of the next tile through the epilogue
    "128,128,13,6,0,0,1,1,256,0,0,2": 16, "128,128,13,6,1,0,1,1,256,0,0,2": 17, "128,128,13,6,0,0,1,1,256,0,1,2": 21,
    "128,128,13,6,1,0,1,1,256,0,1,2": 22, "128,128,13,6,2,0,1,1,256,0,0,2": 0, "128,128,13,6,3,0,1,1,256,0,0,2": 0,
    "128,64,13,6,2,0,1,1,256,0,0,2": 0, "128,64,13,6,3,0,1,1,256,0,0,2": 0,
}
NO_SPILL_SRCS = ("koaf_optim.hip", "koaf_bce.hip", "koaf_wgrad1.hip", "koaf_fwd_s2.hip", "koaf_dgrad_s2.hip", "koaf_fwd1.hip")      # streams: every kernel of these files must report zero spills / scratch
NO_SPILL = re.compile(r"(sgd|rmsprop|adam|adam_hyper|optim_hyper|bce(_sum)?|wgrad1|fwd_s2|dgrad_s2|fwd1)_kernel")
cmds = [c + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/dev/null"]
        for src, c in compile_commands(CS) if src.startswith("koaf_gemm") or src in NO_SPILL_SRCS]
txt = "".join(run_all(cmds, CS))
bad = 0
for b in txt.split("remark: Function Name: ")[1:]:
    name = b.split(" ")[0]
    if NO_SPILL.search(name):
        vg, sp, sc = (int(re.search(p, b).group(1)) for p in (r"VGPRs: (\d+)", r"VGPRs Spill: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)"))
        flag = "   <-- SPILLS" if sp or sc else ""
        bad += bool(flag)
        print(f"{name}  VGPRs {vg}  spilled {sp}  scratch {sc} B{flag}")
        continue
    m = re.search(r"koaf_gemm_kernelI(.*?)EEv", name)
    if not m:
        continue
    args = ",".join(re.findall(r"L[ib](\d+)E", m.group(1)))
    vg, sp, sc = (int(re.search(p, b).group(1)) for p in (r"VGPRs: (\d+)", r"VGPRs Spill: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)"))
    rec = RECORDED.get(args)
    if sp or rec is not None:
        flag = "" if rec is None or sp <= rec + 8 else "   <-- MORE THAN RECORDED (%d)" % rec
        bad += bool(flag)
        print(f"<{args}>  VGPRs {vg}  spilled {sp}  scratch {sc} B{flag}")
sys.exit(1 if bad else 0)
