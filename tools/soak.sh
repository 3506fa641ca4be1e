# Non-default code paths of the exhaustive kernels under the parity tests (one GPU call):
# one-tile and persistent (dynamic schedule) forms.  usage (GPU box): bash tools/soak.sh
cd /root/repo
K="schedules or elimination or batched_exhaustive or full_size or golden_small or random_geometry"
for persist in 0 2; do
  echo -n "persist=$persist: "
  GME_SEA_PERSIST=$persist timeout -k 10 300 python -m pytest tests -x -q -m gpu -k "$K" 2>&1 | tail -1
done
