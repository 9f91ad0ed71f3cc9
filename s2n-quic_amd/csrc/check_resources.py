"""Build-time check of the kernel resource remarks (-Rpass-analysis=kernel-resource-usage, one .res file per .hip).

The AES-GCM kernels reserve their LDS (up to the whole 160 KiB) dynamically, so any static LDS the compiler adds (e.g. a private
array it promotes to LDS because of a runtime index) makes every launch fail with an invalid-allocation error; and
the default variants must not touch scratch memory.  The AES-128-only quad seal / open pair is built for four waves
per SIMD (quad.hip QPP_QUAD_WG128 = 1024 threads, 128 VGPRs): it must report that occupancy, within the same scratch
ceiling.  usage: python3 check_resources.py *.res"""
import re
import sys

SCRATCH_MAX = 32  # bytes per lane, every throughput kernel below (the AES-128 quad pair at 4 waves/SIMD included)
QUAD128_WAVES = 4  # waves per SIMD the AES-128-only quad seal / open instances must reach

bad = []
seen128 = set()
for path in sys.argv[1:]:
    name = None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        if not name:
            continue
        lds = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        scr = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        # kernels that address LDS by absolute offset from 0 (dynamic allocation only)
        dyn_lds = any(k in name for k in ("aes_gcm_quad_kernel", "aes_gcm_quad_rx_kernel", "aes_gcm_wave_kernel",
                                          "aes_gcm_burst_kernel", "txq_server_kernel"))
        # the throughput kernels whose hot loops must not spill (AES-128: the headline)
        default = ("aes_gcm_wave_kernel" in name or re.search(r"aes_gcm_quad_kernelILb[01]ELi10E", name)
                   or re.search(r"aes_gcm_quad_rx_kernelILi10E", name))  # (the AES-128-only receive instance)
        quad128 = re.search(r"aes_gcm_quad_kernelILb([01])ELi10E", name)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if occ and quad128:
            seen128.add(quad128.group(1))
            if int(occ.group(1)) != QUAD128_WAVES:
                bad.append(f"{name}: occupancy {occ.group(1)} waves/SIMD, not {QUAD128_WAVES}")
        if lds and dyn_lds and int(lds.group(1)) != 0:
            bad.append(f"{name}: {lds.group(1)} B of static LDS on top of the dynamic 160 KiB")
        # (a few per-packet spills outside the group loop are tolerated: tools/isa_report.py shows where they are)
        if scr and default and int(scr.group(1)) > SCRATCH_MAX:
            bad.append(f"{name}: {scr.group(1)} B/lane of scratch")
if any(p.endswith("quad.res") for p in sys.argv[1:]) and seen128 != {"0", "1"}:
    bad.append("quad.res: no occupancy remark for the AES-128 quad seal / open pair")
if bad:
    sys.exit("kernel resource check failed:\n  " + "\n  ".join(bad))
