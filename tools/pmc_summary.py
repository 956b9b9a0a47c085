"""Summarize rocprofv3 rocpd .db: per-kernel time and SQ counter ratios."""
import collections
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
names = [r[0] for r in cur.execute("SELECT name FROM sqlite_master WHERE type='table'")]
sfx = [n for n in names if 'kernel_dispatch' in n][0].replace('rocpd_kernel_dispatch_', '')
q = f"""SELECT s.display_name, COUNT(DISTINCT k.id), SUM(k.end-k.start)/1e6
FROM rocpd_kernel_dispatch_{sfx} k
JOIN rocpd_info_kernel_symbol_{sfx} s ON k.kernel_id=s.id GROUP BY 1 ORDER BY 3 DESC LIMIT 12"""
for r in cur.execute(q):
    print(f"{r[2]:9.2f} ms {r[1]:6d} calls  {r[0][:58]}")
if any('pmc_event' in n for n in names):
    # averages over each kernel's LONG dispatches only (at least half
    # its longest): the setup-time probe launches of the solve kernels
    # are tiny and would swamp a per-dispatch mean
    q = f"""SELECT s.display_name, pi.name, AVG(p.value) FROM rocpd_pmc_event_{sfx} p
    JOIN rocpd_kernel_dispatch_{sfx} k ON p.event_id=k.event_id
    JOIN rocpd_info_kernel_symbol_{sfx} s ON k.kernel_id=s.id
    JOIN rocpd_info_pmc_{sfx} pi ON p.pmc_id=pi.id
    JOIN (SELECT kernel_id, MAX(end-start) AS longest
          FROM rocpd_kernel_dispatch_{sfx} GROUP BY kernel_id) m
      ON m.kernel_id=k.kernel_id
    WHERE 2*(k.end-k.start) >= m.longest GROUP BY 1,2"""
    agg = collections.defaultdict(dict)
    for n, c, v in cur.execute(q):
        agg[n.split('(')[0][:34]][c] = v
    for k, v in sorted(agg.items()):
        wc = v.get('SQ_WAVE_CYCLES', 1)
        wa = v.get('SQ_WAIT_ANY', 0) / wc
        wi = v.get('SQ_WAIT_INST_ANY', 0) / wc
        mf = v.get('SQ_VALU_MFMA_BUSY_CYCLES', 0) / (wc * 4)
        if 'SQ_WAVE_CYCLES' in v:
            print(f"{k:36s} waitANY={wa:5.1%} waitINST={wi:5.1%} mfmaBusy={mf:5.1%}")
            # absolute counts per dispatch: a kernel that gets shorter
            # can keep its ratios
            print(f"{k:36s} waveCycles={wc:.4g} "
                  f"mfmaBusyCycles={v.get('SQ_VALU_MFMA_BUSY_CYCLES', 0):.4g}"
                  " per dispatch")
        # memory side, per dispatch (averages): L2 hit rate and the
        # bytes the L2 fetched from beyond it (FETCH_SIZE is in KiB)
        hit = v.get('TCC_HIT_sum', v.get('TCC_HIT'))
        miss = v.get('TCC_MISS_sum', v.get('TCC_MISS'))
        if hit is not None and miss is not None and hit + miss > 0:
            print(f"{k:36s} L2 hit={hit / (hit + miss):5.1%} "
                  f"(hit {hit:.3g}, miss {miss:.3g} per dispatch)")
        if 'FETCH_SIZE' in v:
            print(f"{k:36s} FETCH_SIZE={v['FETCH_SIZE'] / 1024:9.1f} MiB per dispatch")
