#!/usr/bin/env python3
"""Duration distribution (microseconds) of the encoder launch and of rzcc_unit_fallback_kernel in a rocprofv3 kernel trace:
    python tools/dev/slots_trace_summary.py <rocprofv3 output directory>"""
import csv
import glob
import json
import sys

import numpy as np

f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
d = {}
for r in csv.DictReader(open(f)):
    # the sweep's encoder launch: rzcc_sweep.hip's kernel, or rzcc.hip's one-pass spikes-only form in a library without it
    for key, names in (("encoder", ("bandpass_rzcc_sweep_kernel", "bandpass_rzcc_fast_kernel<5, false, true, 64, false")), ("rzcc_unit_fallback_kernel", ("rzcc_unit_fallback_kernel",))):
        if any(n in r["Kernel_Name"] for n in names):
            d.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(json.dumps({k: dict(launches=len(v), min=round(min(v), 1), average=round(float(np.mean(v)), 1), median=round(float(np.median(v)), 1),
                          p95=round(float(np.percentile(v, 95)), 1), max=round(max(v), 1)) for k, v in d.items()}))
