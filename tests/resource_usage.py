"""What the compiler made of the kernels of one `make resource-usage*` target of mygpuraytracer_amd/csrc (hipcc's
-Rpass-analysis=kernel-resource-usage remarks), for the spill tests of the path kernels and the denoiser."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
          ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))


def remarks(target):
    """what `make <target>` printed: the compiler's remarks, each behind the `file:line:column:` of the kernel it describes"""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    assert hipcc, "no hipcc: the library cannot have been built here"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "mygpuraytracer_amd", "csrc"), target, "HIPCC=" + hipcc],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout + r.stderr


def parse_usage(text):
    """{mangled kernel name: {vgprs, scratch, lds, waves}} of every kernel the remarks describe"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def resource_usage(target):
    """{mangled kernel name: {vgprs, scratch, lds, waves}} of every kernel the target compiles"""
    return parse_usage(remarks(target))


def kernels_by_file(text):
    """{source file name: set of mangled kernel names}, from the `file:line:column:` prefix of the "Function Name" remarks"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(?:.*/)?([^/:\s]+):\d+:\d+: remark: Function Name: (\S+)", line)
        if m:
            out.setdefault(m.group(1), set()).add(m.group(2))
    return out


def kernels_named(usage, names):
    """{name: entry of `usage`} for exactly these kernels of the library's anonymous namespaces.  A name is matched whole, as the
    Itanium mangling spells it (<length><name>, closed by E), so "k_atrous_prep" is not also "k_atrous_prep_x"; an instance of a
    template is named with its arguments, e.g. "k_atrous_passILb1ELb0EE".  Each name must be exactly one kernel."""
    found = {}
    for name in names:
        tag = "_GLOBAL__N_1%d%s" % (len(name.split("ILb")[0]), name if "ILb" in name else name + "E")
        hits = [k for k in usage if tag in k]
        assert len(hits) == 1, (name, hits, list(usage))
        found[name] = usage[hits[0]]
    return found
