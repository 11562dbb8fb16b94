# The general plant rollout under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program
# (tools/rollout_sanitize.cpp + the runtime and the kernel text compiled by g++ with -DDOMPC_HOST_EMU): trajectories and argument arrays are
# exact-size heap blocks there, so an index outside them shows up.   bash tools/rollout_sanitize.sh
set -e
cd "$(dirname "$0")/.."
OUT=tests/_hostemu/rollout_sanitize
mkdir -p "$OUT"
python - "$OUT/plant_gen.h" <<'PY'
import sys
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import plant_family_common as pf
from do_mpc_amd.simulator import Simulator
open(sys.argv[1], "w").write(Simulator(pf.build_model("dae"))._lower())
PY
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -DDOMPC_HOST_EMU "-DDOMPC_PLANT_HEADER=\"$PWD/$OUT/plant_gen.h\"" \
  -I do_mpc_amd/csrc tools/rollout_sanitize.cpp do_mpc_amd/csrc/dompc_plant_runtime.cpp -x c++ do_mpc_amd/csrc/dompc_plant.hip -lm -o "$OUT/rollout_sanitize"
"$OUT/rollout_sanitize"
