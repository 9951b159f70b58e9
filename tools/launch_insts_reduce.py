"""tools/launch_insts.sh's reduction: python tools/launch_insts_reduce.py DIR (DIR/ns1, DIR/ns20: rocprofv3 counter collections)"""
import csv, glob, collections, sys
O = sys.argv[1]
res = {}
for ns in (1, 20):
    acc = collections.defaultdict(list)
    for f in glob.glob(O + "/ns%d/**/*counter_collection.csv" % ns, recursive=True) + glob.glob(O + "/ns%db/**/*counter_collection.csv" % ns, recursive=True):   # (ns<k>b: the branch counter's own pass)
        for r in csv.DictReader(open(f)):
            if "k_sfm_step" in r["Kernel_Name"]:
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    res[ns] = {k: (sum(v) / len(v), len(v), min(v), max(v)) for k, v in acc.items()}
    with open(O + "_ns%d_pmc.csv" % ns, "w") as f:   # one row per counter: mean, launches, minimum, maximum over every launch of the step kernel
        f.write("Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value,Dispatches,Min,Max\n")
        for k in sorted(acc):
            f.write('mean,"void cstep::k_sfm_step<0, 1, true, 64, 1, 25, 1>(cstep::KArgs)",%s,%r,%d,%r,%r\n' % (k, res[ns][k][0], res[ns][k][1], res[ns][k][2], res[ns][k][3]))
w = res[20]["SQ_WAVES"][0]
print("per wavefront (%d wavefronts per launch; launches counted: %d at 1 substep, %d at 20):" % (w, res[1]["SQ_WAVES"][1], res[20]["SQ_WAVES"][1]))
for k in sorted(res[20]):
    if k == "SQ_WAVES": continue
    a, b = res[1][k][0] / w, res[20][k][0] / w
    sub = (b - a) / 19
    print("  %-18s 1 substep %9.2f | 20 substeps %9.2f | per substep %8.2f | around the substeps %8.2f" % (k, a, b, sub, a - sub))
