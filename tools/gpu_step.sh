# to be sourced: step <seconds> <command...> runs the command under `timeout -k 10 <seconds>`; on any non-zero status it says so
# on stderr and exits the calling script with that status -- after a fault, abort or time limit nothing more is started on the GPU.
# Redirections stay with the caller: step 600 python3 bench.py ... > $O/x.log 2>&1
step() {
  local limit=$1 status
  shift
  timeout -k 10 "$limit" "$@"
  status=$?
  if [ $status -ne 0 ]; then
    echo "step: status $status from: $*" >&2
    exit $status
  fi
}
