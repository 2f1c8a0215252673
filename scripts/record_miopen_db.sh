#!/bin/bash
# Record MIOpen's user find-db for the stem convolution shapes of the bench (both precisions, training + CAM generation) on an
# MI355X:  [OUT=<dir>] scripts/record_miopen_db.sh  -> $OUT/miopen_db/*.{udb,ufdb}.txt (OUT default: profile_out/), to be merged into acr_wsss_amd/miopen_db/
# (scripts/merge_miopen_db.py).  A fresh, empty user db makes every convolution run MIOpen's full Find once.
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$(mkdir -p "${OUT:-$ROOT/profile_out}" && cd "${OUT:-$ROOT/profile_out}" && pwd)"
export MIOPEN_USER_DB_PATH="$OUT/miopen_db"
rm -rf "$MIOPEN_USER_DB_PATH"; mkdir -p "$MIOPEN_USER_DB_PATH"
cd "$ROOT"
python3 bench.py --full --steps 2 --warmup 2 --no-cpu-baseline --no-roofline > "$OUT/miopen_record.json" 2> "$OUT/miopen_record.err"
echo "rc $? ; $(ls -la $MIOPEN_USER_DB_PATH | tail -3)"
