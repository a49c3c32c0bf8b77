# -DACF_DIAG build of the step library for tools/diag_*.py (stamps; diagnostics only)
set -e
cd "$(dirname "$0")/.."
S=adversarial-collaborative-filtering_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -DACF_DIAG -I include \
  $S/acf_apr.hip $S/acf_plan.hip $S/acf_rank.hip $S/acf_ops.hip -o tools/libacf_apr_diag.so
