#!/bin/bash
# step time over the shortcut branch's stream threshold BR (the matrix had a second dimension, a LOWER row limit for the weight
# gradients' side stream: every value above 0 lost, and that switch was removed from network/plan.py)
for rep in 1 2 3; do for fr in 1 5; do for br in 0 60000 100000; do
  LIDAL_PLAN_BRANCH_ROWS=$br python bench.py --frames $fr --steps 40 --warmup 5 --no-cpu-baseline --no-secondary --no-roofline --no-families --no-variants 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('rep $rep frames $fr branch_rows $br ms/step', d['ms_per_step'])"
done; done; done
