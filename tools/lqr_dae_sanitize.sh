# The design kernel's path for models with algebraic states under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host
# program (tools/lqr_dae_sanitize.cpp + the kernel text compiled by g++ with -DDOMPC_HOST_EMU): LDS regions and argument arrays are plain
# host arrays there, so an index outside them shows up.   bash tools/lqr_dae_sanitize.sh
set -e
cd "$(dirname "$0")/.."
OUT=tests/_hostemu/lqr_dae_sanitize
mkdir -p "$OUT"
python - "$OUT/lqr_gen.h" <<'PY'
import sys
sys.path.insert(0, "tests")
import lqr_dae_common as dc
model, lqr = dc.design("newton", hostemu=True)
open(sys.argv[1], "w").write(lqr.header(model))
PY
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DDOMPC_HOST_EMU "-DDOMPC_LQR_HEADER=\"$PWD/$OUT/lqr_gen.h\"" \
  -I do_mpc_amd/csrc tools/lqr_dae_sanitize.cpp -x c++ do_mpc_amd/csrc/dompc_lqr.hip -lm -o "$OUT/lqr_dae_sanitize"
"$OUT/lqr_dae_sanitize"
