# The host device layer (csrc/dompc_host.h) under AddressSanitizer (leak detection on) and UndefinedBehaviorSanitizer, as a stand-alone
# host program: tools/host_layer_sanitize.cpp + csrc/dompc_ampc_runtime.cpp + the kernel text of csrc/dompc_ampc.hip compiled by g++ with
# -DDOMPC_HOST_EMU.  Creates that fail, a refused upload, staging that grows and is reused, the Jacobian entry: an access outside an
# allocation or a block that nobody frees shows up.   bash tools/host_layer_sanitize.sh
set -e
cd "$(dirname "$0")/.."
OUT=tests/_hostemu/host_layer_sanitize
mkdir -p "$OUT"
HASH=$(python - "$OUT/ampc_gen.h" <<'PY'
import sys
from do_mpc_amd import lowering
hdr = lowering.lower_ampc(6, 2, 1, 50, "tanh", "linear", True)
open(sys.argv[1], "w").write(hdr)
print(hdr.rsplit('AMPC_MODEL_HASH "', 1)[1].split('"')[0])
PY
)
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -DDOMPC_HOST_EMU \
  "-DDOMPC_AMPC_HEADER=\"$PWD/$OUT/ampc_gen.h\"" -I do_mpc_amd/csrc tools/host_layer_sanitize.cpp do_mpc_amd/csrc/dompc_ampc_runtime.cpp \
  -x c++ do_mpc_amd/csrc/dompc_ampc.hip -lm -o "$OUT/host_layer_sanitize"
ASAN_OPTIONS=detect_leaks=1 "$OUT/host_layer_sanitize" "$HASH"
