# usage: bash tools/gpu_ab.sh <outdir-name> <variant-file>
# Each non-empty line of the variant file: "<label> | <ENV=... ENV=...> | <bench args>"; runs bench.py once per line (same box,
# back to back) and prints label + value + ms/step (+ roofline and checksum where the line has them; the training bench: phases
# and losses).  One log per label in the out-dir.  A variant that fails ends the A/B: later variants are not started.
cd "$(dirname "$0")/.."
. tools/gpu_step.sh
export TMPDIR=/tmp
O=gpurun_out/$1; mkdir -p $O
exec 3>&2; trap 's=$?; [ $s -eq 0 ] || echo "gpu_ab: stopped with status $s at \"$label\" (log: $O/$label.log)" >&3' EXIT   # (fd 3: step's own message follows the caller's redirection into the log)
while IFS='|' read -r label envs bargs; do
  label=$(echo $label); [ -z "$label" ] && continue
  step 600 env $envs ${PYTHON:-python3} bench.py --cpu-seconds 0 $bargs < /dev/null > $O/$label.log 2>&1
  python3 - "$O/$label.log" "$label" <<'PY'
import json, sys
line = None
for l in open(sys.argv[1], errors="replace"):
    if l.startswith("{"):
        line = l
if line is None:
    print("%-28s no result line" % sys.argv[2]); sys.exit(1)
j = json.loads(line)
out = "%-28s %9.1f %s %8.3f ms/step" % (sys.argv[2], j["value"], j["unit"], j["ms_per_step"])
r, c = j.get("roofline") or {}, j.get("config") or {}
if r:
    out += "  dom %s frac %.4f" % (r.get("kernel"), r.get("frac", 0))
if "checksum" in c:
    out += "  checksum %s" % (c["checksum"],)
if "phase_ms_per_step" in c:
    out += "  %s  loss %.6f -> %.6f" % (c["phase_ms_per_step"], c["loss_first"], c["loss_last"])
print(out)
PY
  [ $? -eq 0 ] || exit 1
done < $2
