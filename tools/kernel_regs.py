"""register / scratch / LDS report from a hipcc -S listing: python tools/kernel_regs.py file.s [substring]
(hipcc -S --cuda-device-only --offload-arch=gfx950 with the flags of csrc/Makefile; pipe through c++filt for readable names)"""
import re
import sys
txt = open(sys.argv[1]).read()
flt = sys.argv[2] if len(sys.argv) > 2 else ""
# the compiler's comment block behind every kernel, in the order of the kernels: SGPRs (with VCC etc.), VGPRs, AGPRs
info = re.findall(r"; TotalNumSgprs: (\d+)\n; NumVgprs: (\d+)\n(?:; NumAgprs: (\d+)\n)?", txt)
for k, m in enumerate(re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S)):
    name, body = m.group(1), m.group(2)
    if flt not in name:
        continue
    def get(key):
        r = re.search(r"\.amdhsa_%s (\S+)" % key, body)
        return r.group(1) if r else "?"
    sgpr, vgpr, agpr = info[k] if k < len(info) else ("?", "?", "?")
    print("%-100s vgpr=%-4s accum_off=%-4s scratch=%-5s sgpr=%-4s arch_vgpr=%-4s agpr=%-4s static_lds=%s" % (
        name.replace("_ZN2lg10sgemm_mfmaI", "sgemm<").replace("EEvNS_8GemmArgsE", ">"),
        get("next_free_vgpr"), get("accum_offset"), get("private_segment_fixed_size"), sgpr, vgpr, agpr or "0", get("group_segment_fixed_size")))
