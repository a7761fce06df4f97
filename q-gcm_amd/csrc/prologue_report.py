"""Per-kernel prologue report from the device assembly (hipcc --cuda-device-only -S), written next to the library by
the Makefile and read by tests/test_gpu_prologue_args.py.  One line per kernel:
  <symbol> preload=<SGPRs preloaded from the kernarg segment> scalar_waits=<waits for scalar loads before the first
  vector load in program text> scalar_loads=<scalar loads issued before it> vgpr=<n> sgpr=<n> scratch=<bytes per lane>
  occupancy=<waves per SIMD>
A kernel with preloaded arguments starts with a compatibility header (scalar loads of the same arguments, a wait and a
branch) that only runs where the firmware does not preload; the count starts behind it."""
import re
import sys


def report(lines):
    out, cur, body = [], None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+|\w+):\s*; @", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        body.append(ln)
        if ln.startswith("; Occupancy:"):
            txt = "".join(body)
            def field(name):
                f = re.search(r"\.amdhsa_%s (\d+)" % name, txt)
                return int(f.group(1)) if f else 0
            pre = field("user_sgpr_kernarg_preload_length")
            code = body[:next(i for i, b in enumerate(body) if b.startswith("\t.section") or b.startswith("\t.amdhsa_kernel") or ".amdhsa_kernel" in b)]
            if pre:
                for i, b in enumerate(code):
                    if re.match(r"\s+s_branch\b", b):
                        code = code[i + 1:]
                        break
            waits = loads = 0
            for b in code:
                ins = b.split(";")[0].strip()
                if re.match(r"(global|buffer|flat|scratch)_load", ins):
                    break
                if re.match(r"s_(buffer_)?load_", ins):
                    loads += 1
                if ins.startswith("s_waitcnt") and "lgkmcnt(0)" in ins and loads:
                    waits += 1
            scr = re.search(r"; ScratchSize: (\d+)", txt)
            vg = re.search(r"; NumVgprs: (\d+)", txt)
            sg = re.search(r"; TotalNumSgprs: (\d+)", txt)
            occ = re.search(r"; Occupancy: (\d+)", txt)
            out.append("%s preload=%d scalar_waits=%d scalar_loads=%d vgpr=%s sgpr=%s scratch=%s occupancy=%s" % (
                cur, pre, waits, loads, vg.group(1) if vg else "?", sg.group(1) if sg else "?", scr.group(1) if scr else "?",
                occ.group(1) if occ else "?"))
            cur = None
    return out


if __name__ == "__main__":
    for ln in report(open(sys.argv[1])):
        print(ln)
