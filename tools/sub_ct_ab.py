"""A/B of the multi-pass sub-transform kernels (witness_sub_ct 0, the generic kernel, vs 2, the wide kernel) at the headline shape: per-kernel ms of one proof."""
import os
import subprocess
import sys

for v in sys.argv[1:] or ["0", "2"]:
    env = dict(os.environ, RS_TUNING="witness_sub_ct=" + v)
    out = subprocess.run([sys.executable, "tools/headline_probe.py", "16", "13", "2"], env=env, capture_output=True, text=True)
    print("witness_sub_ct", v)
    print("\n".join(ln for ln in out.stdout.splitlines() if ln.startswith("proof") or "sub_ntt" in ln or "Error" in ln), out.stderr[-400:] if out.returncode else "")
