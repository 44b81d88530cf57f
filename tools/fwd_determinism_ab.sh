cd $GRAFT_REPO_ROOT
for s in "X=0" "TMI_GEMM_GENERIC=1"; do
  echo "== $s"; env $s python tools/fwd_determinism.py 2>&1 | grep "bf16 model 0"
done
