# A/B of two builds of the library on the same box: dedalus_amd/csrc/libdedalus_hip_base.so (DDH_LIB) against the in-tree build
AB=${AB_OUT:-ab_out}
mkdir -p $AB
python -m pytest tests/test_gpu_wave_transforms.py -q -m gpu -x 2>&1 | tail -2
for i in 1 2; do
DDH_LIB=$PWD/dedalus_amd/csrc/libdedalus_hip_base.so python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $AB/base$i.json 2> $AB/base$i.err
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $AB/new$i.json 2> $AB/new$i.err
done
python - $AB <<'PY'
import json, sys
for n in ("base1","new1","base2","new2"):
    try:
        d=json.loads(open("%s/%s.json"%(sys.argv[1],n)).read().strip().splitlines()[-1])
        print(n, "steps/s %.3f ms %.2f chk %.15g frac %.3f"%(d["value"],d["ms_per_step"],d["checksum_b_c_l2"],d["roofline"]["frac"]))
        print("   ", {k:(round(v["avg_ms"],3)) for k,v in d["kernels"].items()})
    except Exception as e:
        print(n,"unreadable",e); print(open("%s/%s.err"%(sys.argv[1],n)).read()[-2000:])
PY
