# sourced by the profiling scripts: ROOT = the repository, OUT = the directory they write to (SR_PROF_OUT, default <repository>/prof_out)
ROOT=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
mkdir -p "${SR_PROF_OUT:-$ROOT/prof_out}"
OUT=$(cd "${SR_PROF_OUT:-$ROOT/prof_out}" && pwd)
export SR_PROF_OUT=$OUT
