"""The reader of a rocprofv3 --kernel-trace run, written once for the study tools' --kernel-report modes.

read_trace(DIR) finds the trace below DIR and returns its launches in start order as (kernel name, device time in us).  A template
instantiation appears under three spellings, depending on the profiler's version and on whether it demangles: `k<true, 1>`,
`k<true,1>` and the mangled `kILb1ELi1E`; is_instance / durations match all of them in one place."""
import csv
import glob
import os


def read_trace(d):
    """[(Kernel_Name, us)] of the first *kernel_trace.csv below d, sorted by start time"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    with open(f) as fi:
        rows = list(csv.DictReader(fi))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]


def short_name(name):
    """a demangled name without its arguments, `void` and the rt:: namespace"""
    return name.split("(")[0].replace("rt::", "").replace("void ", "")


def is_instance(name, kernel, *args):
    """whether a trace name is kernel<args...> (bool and int template arguments) under any of its spellings; a bool may also be
    printed as 0 / 1"""
    texts = [[str(a).lower(), str(int(a))] if isinstance(a, bool) else [str(a)] for a in args]
    spelled = [[]]
    for t in texts:
        spelled = [s + [x] for s in spelled for x in t]
    mangled = kernel + "I" + "".join("Lb%dE" % a if isinstance(a, bool) else "Li%dE" % a for a in args) + "E"
    return mangled in name or any("%s<%s>" % (kernel, sep.join(s)) in name for s in spelled for sep in (", ", ","))


def durations(events, kernel, *args):
    """the times, in trace order, of the launches whose name holds `kernel`, or, with template arguments, of that instantiation"""
    return [us for name, us in events if (is_instance(name, kernel, *args) if args else kernel in name)]
