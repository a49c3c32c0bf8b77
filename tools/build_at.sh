# Build libacf_apr.so from an older commit's sources into tools/libacf_apr_<rev>.so
# (same-box A/Bs against the current build: tools/large_line.py, ACF_LARGE_LINE_LIB).
# usage: bash tools/build_at.sh <rev>
set -e
cd "$(dirname "$0")/.."
rev=$1
tmp=$(mktemp -d)
mkdir -p $tmp/include $tmp/csrc
git show $rev:include/acf_apr.h > $tmp/include/acf_apr.h
for f in $(git ls-tree --name-only $rev adversarial-collaborative-filtering_amd/csrc/); do
  case $f in *.hip|*.h) git show $rev:$f > $tmp/csrc/$(basename $f);; esac
done
srcs=
for s in acf_apr acf_plan acf_rank acf_ops; do  # the library's sources that exist at $rev (not before their splits)
  [ -f $tmp/csrc/$s.hip ] && srcs="$srcs $tmp/csrc/$s.hip"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -I $tmp/include \
  $srcs -o tools/libacf_apr_$rev.so
rm -rf $tmp
echo tools/libacf_apr_$rev.so
