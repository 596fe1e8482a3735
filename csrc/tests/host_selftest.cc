// Standalone self-test of the native host runtime (no torch, no GPU), built
// plain and under AddressSanitizer / ThreadSanitizer by
// `python build_native.py --sanitize address|thread` (the
// reference has no sanitizer targets; its host code had real races). It
// exercises every component that owns memory or threads: the LZ4 codec, the
// CRB row-block format, the text parsers, InputSplit part alignment (text
// and RecordIO), the multi-threaded ordered ThreadedReader / MinibatchIter,
// the conf parser, the WorkloadPool under concurrent workers and the
// control-plane transport (Van) with live reader threads; and the pure
// arithmetic of the exact AUC, of the two store guards' plans, of the
// localize job's bookkeeping and of the GBDT histogram task lists and level
// tables; and the host-thread AUC's job ledger under test workers.
#include <cmath>
#include <limits>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "host/auc_host.h"
#include "host/auc_jobs.h"
#include "host/common.h"
#include "host/gbdt_hist_plan.h"
#include "host/gbdt_level_plan.h"
#include "host/gbdt_node_rule.h"
#include "host/gbdt_objective.h"
#include "host/io.h"
#include "host/json.h"
#include "host/linear_guard_plan.h"
#include "host/localize_plan.h"
#include "host/parsers.h"
#include "host/psx_plan.h"
#include "host/store_guard_plan.h"
#include "host/van.h"
#include "host/workload_pool.h"

using namespace wh::host;

static int g_fail = 0;
#define EXPECT(c)                                                         \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

static void test_lz4() {
  std::mt19937 rng(1);
  for (int kind = 0; kind < 3; ++kind) {
    for (int n : {0, 1, 7, 100, 4096, 300000}) {
      std::string src(n, '\0');
      for (int i = 0; i < n; ++i)
        src[i] = kind == 0 ? (char)rng() : kind == 1 ? (char)('a' + i % 7) : (char)(i / 1000);
      std::string dst(LZ4CompressBound(n) + 16, '\0');
      const int c = LZ4Compress(src.data(), &dst[0], n, (int)dst.size());
      EXPECT(c >= 0);
      std::string back(n + 8, '\0');
      const int d = LZ4Decompress(dst.data(), &back[0], c, n);
      EXPECT(d == n);
      EXPECT(std::memcmp(back.data(), src.data(), n) == 0);
    }
  }
  // malformed input must fail cleanly, never write out of bounds
  std::string junk(64, '\xff'), out(16, '\0');
  EXPECT(LZ4Decompress(junk.data(), &out[0], (int)junk.size(), (int)out.size()) < 0);
}

static RowBlock random_block(size_t rows, bool with_val, uint32_t seed) {
  std::mt19937_64 rng(seed);
  RowBlock b;
  for (size_t r = 0; r < rows; ++r) {
    b.label.push_back((float)(rng() % 2));
    const int len = 1 + (int)(rng() % 40);
    for (int j = 0; j < len; ++j) {
      b.index.push_back(rng());
      if (with_val) b.value.push_back((float)(rng() % 100) / 7.f);
    }
    b.offset.push_back((int64_t)b.index.size());
  }
  return b;
}

static bool same(const RowBlock& a, const RowBlock& b) {
  return a.label == b.label && a.offset == b.offset && a.index == b.index && a.value == b.value &&
         a.weight == b.weight;
}

static void test_crb() {
  for (bool v : {false, true}) {
    RowBlock b = random_block(1000, v, 7), d;
    const std::string enc = CRBEncode(b);
    CRBDecode(enc.data(), enc.size(), &d);
    EXPECT(same(b, d));
  }
}

static void test_parsers() {
  RowBlock b;
  const std::string svm = "1 3:0.5 9:1\n0 2:2\n\n1 7\n";
  ParseLibSVM(svm.data(), svm.data() + svm.size(), &b);
  EXPECT(b.size() == 3 && b.nnz() == 4);
  EXPECT(b.index[0] == 3 && b.index[3] == 7);
  const std::string crit = "1\t5\t\t3" + std::string(10, '\t') + "\tdeadbeef" +
                           std::string(25, '\t') + "\n";
  ParseCriteo(crit.data(), crit.data() + crit.size(), true, &b);
  EXPECT(b.size() == 1 && b.nnz() == 3);
  EXPECT((b.index[2] >> 54) == 13);  // first categorical field
  const std::string adfea = "1 2 1 5:3 9:4\n";
  ParseAdfea(adfea.data(), adfea.data() + adfea.size(), &b);
  EXPECT(b.size() == 1 && b.nnz() == 2);
}

static std::string tmpfile(const char* name) {
  const char* d = std::getenv("TMPDIR");
  return std::string(d && *d ? d : "/tmp") + "/wh_selftest_" + name;
}

static void test_splits_and_reader() {
  // text: every line lands in exactly one of n parts, in order
  const std::string path = tmpfile("text.svm");
  {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    for (int i = 0; i < 20000; ++i) std::fprintf(f, "%d %d:1 %d:2\n", i % 2, i, i + 1);
    std::fclose(f);
  }
  for (int n : {1, 3, 16}) {
    std::vector<uint64_t> seen;
    for (int k = 0; k < n; ++k) {
      BlockReader r(path, k, n, "libsvm");
      RowBlock b;
      while (r.Next(&b))
        for (size_t i = 0; i < b.size(); ++i) seen.push_back(b.index[b.offset[i]]);
    }
    EXPECT(seen.size() == 20000);
    for (size_t i = 0; i < seen.size(); ++i) EXPECT(seen[i] == i);
  }
  // RecordIO (CRB): parts align to records, every record once
  const std::string crb = tmpfile("blocks.crb");
  std::vector<RowBlock> blocks;
  {
    RecordIOWriter w(crb);
    for (int i = 0; i < 50; ++i) {
      blocks.push_back(random_block(100 + i, i % 2 == 0, 100 + i));
      w.WriteRecord(CRBEncode(blocks.back()));
    }
    w.Close();
  }
  for (int n : {1, 4, 13}) {
    size_t got = 0;
    for (int k = 0; k < n; ++k) {
      BlockReader r(crb, k, n, "crb");
      RowBlock b;
      while (r.Next(&b)) {
        EXPECT(got < blocks.size() && same(b, blocks[got]));
        ++got;
      }
    }
    EXPECT(got == blocks.size());
  }
  // many parser threads hand out chunks in read order
  std::vector<std::vector<uint64_t>> runs;
  for (int nt : {1, 8}) {
    ThreadedReader tr(path, 0, 1, "libsvm", nt);
    RowBlock b;
    std::vector<uint64_t> ids;
    while (tr.Next(&b)) ids.insert(ids.end(), b.index.begin(), b.index.end());
    runs.push_back(ids);
  }
  EXPECT(runs[0] == runs[1] && runs[0].size() == 40000);
  // early destruction with workers still running must not leak or race
  for (int i = 0; i < 5; ++i) {
    ThreadedReader tr(path, 0, 1, "libsvm", 8);
    RowBlock b;
    tr.Next(&b);
  }
  // minibatches with the shuffle buffer and negative sampling
  MinibatchIter it(path, 0, 1, "libsvm", 1000, 5000, 0.5f, 3, 4);
  size_t rows = 0;
  while (it.Next()) rows += it.Value().size();
  EXPECT(rows > 12000 && rows < 18000);  // all positives + about half the negatives
  std::remove(path.c_str());
  std::remove(crb.c_str());
}

static void test_conf() {
  auto items = ParseConf("# c\nminibatch = 1000\nembedding {\n dim = 16\n}\nname: \"x y\"\n");
  EXPECT(items.size() == 3);
  EXPECT(items[0].key == "minibatch" && items[0].value == "1000");
  EXPECT(items[1].kind == 'm' && items[1].children.size() == 1);
  EXPECT(items[2].kind == 's' && items[2].value == "x y");
}

static void test_pool_concurrent() {
  WorkloadPool pool(true, 5, 2.0, 5.0, 10, 0.05);
  std::vector<std::string> files;
  for (int i = 0; i < 20; ++i) files.push_back("f" + std::to_string(i));
  pool.Add(files, 10);
  std::atomic<int> done{0};
  std::vector<std::thread> th;
  for (int w = 0; w < 8; ++w) {
    th.emplace_back([&, w] {
      const std::string me = "worker-" + std::to_string(w);
      Assignment a;
      int resets = 0;
      while (pool.Get(me, &a)) {
        if (w == 3 && resets < 3) {
          ++resets;
          pool.Reset(me);  // a failure: the part goes back to the pool
          continue;
        }
        pool.FinishOne(me, a.filename, a.k);
        done.fetch_add(1);
      }
    });
  }
  for (auto& t : th) t.join();
  EXPECT(pool.IsFinished());
  EXPECT(pool.num_finished() == 200);
}

static void test_json() {
  // the control-plane messages: Python json.dumps output in, ours out
  Json d = Json::Parse(
      "{\"msg\": \"request\", \"finished\": {\"file\": \"a\\\"b\\u00e9\", \"k\": 3},"
      " \"data\": [1.5, -2e-3, 0, NaN], \"files\": [], \"x\": null, \"ok\": true}");
  EXPECT(d["msg"].str() == "request");
  EXPECT(d["finished"]["k"].num() == 3);
  EXPECT(d["finished"]["file"].str() == "a\"b\xc3\xa9");
  const auto v = d["data"].nums();
  EXPECT(v.size() == 4 && v[0] == 1.5 && v[1] == -2e-3 && v[3] != v[3]);
  EXPECT(d["files"].strs().empty() && d["x"].is_null() && d["ok"].truthy());
  EXPECT(!d["missing"].truthy());
  Json o = Json::Obj().set("cmd", Json::Str("workload")).set("file", Json::Null())
               .set("k", Json::Num(7)).set("w", Json::Num(0.25));
  Json back = Json::Parse(o.Dump());
  EXPECT(back["cmd"].str() == "workload" && back["file"].is_null());
  EXPECT(back["k"].num() == 7 && back["w"].num() == 0.25);
  bool threw = false;
  try {
    Json::Parse("{\"a\": }");
  } catch (const std::exception&) {
    threw = true;
  }
  EXPECT(threw);
}

static void test_van() {
  // control-plane transport: 4 clients x 200 frames into one listener, and
  // replies back, with every connection's reader thread live
  Van server;
  const int port = server.Listen(0);
  EXPECT(port > 0);
  std::vector<std::thread> th;
  std::atomic<int> replies{0};
  for (int c = 0; c < 4; ++c) {
    th.emplace_back([&, c] {
      Van cl;
      const std::string me = "client-" + std::to_string(c);
      cl.Connect("127.0.0.1", port, me, 10.0);
      for (int i = 0; i < 200; ++i) EXPECT(cl.Send("scheduler", me + ":" + std::to_string(i)));
      std::string from, msg;
      int got = 0;
      while (got < 200 && cl.Recv(10.0, &from, &msg)) ++got;
      replies.fetch_add(got);
      cl.Close();
    });
  }
  int n = 0;
  std::string from, msg;
  while (n < 800 && server.Recv(10.0, &from, &msg)) {
    if (msg == "__closed__") continue;  // a client that already got all its acks
    ++n;
    EXPECT(msg.rfind(from + ":", 0) == 0);
    EXPECT(server.Send(from, "ack"));
  }
  EXPECT(n == 800);
  for (auto& t : th) t.join();
  EXPECT(replies.load() == 800);
  server.Close();
}

// the host AUC against an O(n^2) count of the same definition (key order:
// score bits, then index)
static void test_auc() {
  std::mt19937 rng(5);
  std::vector<uint64_t> ws;
  for (int n : {1, 2, 3, 17, 400, 3000}) {
    for (int kind = 0; kind < 3; ++kind) {
      std::vector<float> p(n), l(n);
      for (int i = 0; i < n; ++i) {
        p[i] = kind == 0 ? (float)(rng() % 1000) / 999.f
                         : kind == 1 ? (float)(rng() % 4) * (rng() % 2 ? -1.f : 1.f) : 0.5f;
        l[i] = (rng() % 3) == 0 ? 1.f : 0.f;
      }
      uint64_t tot = 0, tp = 0;
      for (int i = 0; i < n; ++i) tp += l[i] > 0.f;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          if (!(l[i] > 0.f) || l[j] > 0.f) continue;
          const uint32_t a = wh::auc_ord_bits(p[i]), b = wh::auc_ord_bits(p[j]);
          tot += a < b || (a == b && i < j);
        }
      double want = 1.0;
      if (tp != 0 && tp != (uint64_t)n) {
        const double r = (double)tot / ((double)tp * (double)(n - tp));
        want = r < 0.5 ? 1 - r : r;
      }
      EXPECT(wh::auc_exact_host(p.data(), l.data(), n, ws) == want);
    }
  }
}

// The host-thread AUC's job ledger (host/auc_jobs.h) as the binding drives
// it, with the test in the binding's place: it owns what ev and buf point to,
// gives fresh jobs their cap, and its workers finish jobs with results it
// supplies. Workers end on sentinel jobs (the product's never end).
static void test_auc_jobs() {
  using namespace std::chrono_literals;
  // Submission-order fold: 40 jobs over two targets, three workers. Each
  // group of three jobs finishes in reverse (job i waits at the gate until
  // the later jobs of its group have finished), so every fold happens with
  // jobs finished out of order; the sums must still be the left-to-right ones.
  {
    const int N = 40;
    const double vals[4] = {1e16, 1.0, -1e16, 3.0};
    struct Item { double r; int target; };
    std::vector<Item> items(N);
    for (int i = 0; i < N; ++i) items[i] = {vals[i / 2 % 4], i % 2};  // each target: vals, 5 times
    int tgt[2], stop;  // (their addresses name the targets)
    double fwd[2] = {0, 0}, rev[2] = {0, 0};
    for (int i = 0; i < N; ++i) fwd[items[i].target] += items[i].r;
    for (int i = N - 1; i >= 0; --i) rev[items[i].target] += items[i].r;
    EXPECT(fwd[0] == 19 && rev[0] == 20 && fwd[1] == 19 && rev[1] == 20);  // order shows

    wh::AucJobs jobs(64);
    std::mutex gm;
    std::condition_variable gcv;
    std::vector<char> fin(N, 0);
    std::vector<int> order;
    auto worker = [&] {
      for (;;) {
        wh::AucJob* j = jobs.take();
        if (j->target == &stop) {
          jobs.finish(j, 0);
          return;
        }
        const int i = (int)(static_cast<Item*>(j->ev) - items.data());
        {
          std::unique_lock<std::mutex> lk(gm);
          gcv.wait(lk, [&] {
            for (int k = i + 1; k < std::min(N, i / 3 * 3 + 3); ++k)
              if (!fin[k]) return false;
            return true;
          });
        }
        jobs.finish(j, items[i].r);
        std::lock_guard<std::mutex> lk(gm);
        fin[i] = 1;
        order.push_back(i);
        gcv.notify_all();
      }
    };
    std::vector<std::thread> th;
    for (int w = 0; w < 3; ++w) th.emplace_back(worker);
    for (int i = 0; i < N + 3; ++i) {
      wh::AucJob* j = jobs.acquire(1);
      EXPECT(j->n == 1 && !j->done);
      if (!j->cap) j->cap = 1;
      j->ev = i < N ? &items[i] : nullptr;
      jobs.submit(j, i < N ? (const void*)&tgt[items[i].target] : &stop);
    }
    for (int t = 0; t < 2; ++t) {  // (blocks until the target's last job folds)
      double s = -1;
      EXPECT(jobs.join(&tgt[t], &s) && s == fwd[t]);
    }
    for (auto& t : th) t.join();
    EXPECT((int)order.size() == N && order[0] == 2 && order[1] == 1 && order[2] == 0);
  }
  // Back-pressure, recycling and join, single-stepped: no workers, the test
  // takes and finishes the jobs itself
  {
    wh::AucJobs jobs(4);
    int t, u, never;
    wh::AucJob* j[4];
    for (int k = 0; k < 4; ++k) {
      j[k] = jobs.acquire(10);
      EXPECT(j[k]->cap == 0);  // fresh
      j[k]->cap = 100 * (k + 1);
      jobs.submit(j[k], &t);
    }
    for (int k = 0; k < 4; ++k) EXPECT(jobs.take() == j[k]);  // in submission order
    std::atomic<bool> got{false};
    wh::AucJob* fifth = nullptr;
    std::thread sub([&] {
      fifth = jobs.acquire(150);
      got = true;
    });
    std::this_thread::sleep_for(50ms);
    EXPECT(!got);  // four unfolded jobs: the fifth acquire waits
    jobs.finish(j[1], 2.0);
    std::this_thread::sleep_for(50ms);
    EXPECT(!got);  // job 2 is finished but not at the head of the line: no space
    jobs.finish(j[0], 1.0);  // folds jobs 1 and 2
    sub.join();
    EXPECT(got && fifth == j[1]);  // free: {100, 200}; the first with cap >= 150
    jobs.finish(j[3], 4.0);
    jobs.finish(j[2], 3.0);  // free: caps {100, 300, 400}
    wh::AucJob* big = jobs.acquire(1000);  // larger than every free job: a fresh one
    EXPECT(big->cap == 0 && big->n == 1000);
    for (int k = 0; k < 4; ++k) EXPECT(big != j[k]);
    EXPECT(jobs.acquire(250) == j[2]);  // skips the smaller free job
    EXPECT(jobs.acquire(1) == j[0]);
    for (int k = 0; k < 4; ++k) EXPECT(j[k]->cap == 100 * (k + 1));  // none regrown

    double s = -1;
    EXPECT(!jobs.join(&never, &s) && s == -1);  // never submitted: at once
    EXPECT(jobs.join(&t, &s) && s == 10.0);     // all folded
    EXPECT(!jobs.join(&t, &s));                 // and forgotten
    // unfolded jobs: join waits for the last fold (submitted: fifth, big, j[2])
    big->cap = 1000;
    jobs.submit(fifth, &u);
    jobs.submit(big, &u);
    jobs.submit(j[2], &u);
    std::atomic<bool> joined{false};
    double su = -1;
    bool had = false;
    std::thread joiner([&] {
      had = jobs.join(&u, &su);
      joined = true;
    });
    EXPECT(jobs.take() == fifth && jobs.take() == big && jobs.take() == j[2]);
    jobs.finish(j[2], 4.0);
    jobs.finish(fifth, 1.0);  // folds only itself: big is unfinished
    std::this_thread::sleep_for(50ms);
    EXPECT(!joined);
    jobs.finish(big, 2.0);
    joiner.join();
    EXPECT(had && su == 7.0);
  }
}

// the store guard's plan as the native guard drives it: four opens from a
// table of 1024 slots and a V slab of 64 rows at max_load 0.7 (expected
// values from kv/__init__.py StoreGuard.before_open on a stub store)
static void test_store_guard_plan() {
  wh::StoreGuardPlan p;
  int64_t cap = 1024, vcap = 64;
  auto open = [&](int64_t n) {
    cap = wh::grown_cap(p.need(n), cap, 0.7);
    if (p.vneed(n) > vcap) vcap = wh::grown_vcap(p.vneed(n), vcap);
    p.opened(n);
  };
  auto is = [&](int64_t c, int64_t v, int64_t since, int64_t r0, int64_t r1) {
    return cap == c && vcap == v && p.since == since && p.recent[0] == r0 && p.recent[1] == r1;
  };
  open(600);
  EXPECT(is(1024, 1024, 600, 0, 600));
  open(300);
  EXPECT(is(2048, 2048, 900, 600, 300));
  p.summarised(850, 700);
  EXPECT(p.keys == 850 && p.vused == 700 && p.since == 0);
  open(10);
  EXPECT(is(2048, 2048, 10, 300, 10));
  EXPECT(p.vneed(1000) == 2020);  // at most 2048: the slab must not grow
  open(1000);
  EXPECT(is(4096, 2048, 1010, 10, 1000));
  // the load bound is compared in floating point: 716 < 0.7 * 1024 = 716.8
  EXPECT(wh::grown_cap(716, 1024, 0.7) == 1024);
  EXPECT(wh::grown_cap(717, 1024, 0.7) == 2048);
  EXPECT(wh::grown_vcap(1, 0) == 1 && wh::grown_vcap(64, 64) == 64 && wh::grown_vcap(65, 64) == 128);
}

// LinearStep's guard plan as the step drives it (guard_before: grow_target;
// guard_after: due; guard_read: summarised), at cap = 4096 and max_load 0.7.
// This guard has no Python twin: the expected values are worked out here from
// the rule "no summary when unforced, not the 8th unforced call, and
// bound + 8 n < 0.9 * max_load * cap", with max_load * cap = 2867.2 and
// 0.9 * 2867.2 = 2580.48, and bound = base_keys + (issued - base_issued).
static void test_linear_guard_plan() {
  const int64_t cap = 4096;
  const double ml = 0.7;
  EXPECT(wh::LinearGuardPlan::kGuardEvery == 8);
  {
    // steady cadence: opens of 10 ids from an empty table. After call k the
    // bound is 10 k, and 10 k + 80 <= 240 is far below 2580.48: only the
    // counter makes a summary due, at calls 8 and 16
    wh::LinearGuardPlan p;
    for (int k = 1; k <= 16; ++k) EXPECT(p.due(10, cap, ml, false) == (k == 8 || k == 16));
    EXPECT(p.issued == 160 && p.bound() == 160 && p.step == 16);
    // a summary applied: 50 keys when 80 ids had been issued (ids repeat
    // across minibatches, so 50 < 80); 80 more were issued since
    p.summarised(50, 80);
    EXPECT(p.base_keys == 50 && p.base_issued == 80 && p.bound() == 50 + 80);
    // a stale summary (stamped 40, read after the one stamped 80) is dropped
    p.summarised(45, 40);
    EXPECT(p.base_keys == 50 && p.base_issued == 80 && p.bound() == 130);
    // one with the same stamp (guard_sync's forced summary of 0 ids) counts
    p.summarised(48, 80);
    EXPECT(p.base_keys == 48 && p.bound() == 128);
  }
  {
    // near the load limit: a base of 2500 keys. Call k: bound = 2500 + 10 k,
    // and 2500 + 10 + 80 = 2590 >= 2580.48 already at k = 1: every call is due
    wh::LinearGuardPlan p;
    p.summarised(2500, 0);
    for (int k = 1; k <= 7; ++k) EXPECT(p.due(10, cap, ml, false));
    EXPECT(p.bound() == 2570);
    // both sides of 0.9 * lim on a first call (the counter says no): with
    // n = 10 the sum is base + 10 + 80; 2490 + 90 = 2580 < 2580.48 is not
    // due, 2491 + 90 = 2581 is
    wh::LinearGuardPlan lo, hi;
    lo.summarised(2490, 0);
    hi.summarised(2491, 0);
    EXPECT(!lo.due(10, cap, ml, false));
    EXPECT(hi.due(10, cap, ml, false));
  }
  {
    // a forced call (guard_sync: n = 0) is due and leaves the cadence alone:
    // three unforced calls, the forced one, then calls 4..7 are not due and
    // the 8th unforced call is
    wh::LinearGuardPlan p;
    for (int k = 1; k <= 3; ++k) EXPECT(!p.due(10, cap, ml, false));
    EXPECT(p.due(0, cap, ml, true));
    EXPECT(p.step == 3 && p.issued == 30);
    for (int k = 4; k <= 7; ++k) EXPECT(!p.due(10, cap, ml, false));
    EXPECT(p.due(10, cap, ml, false));
    EXPECT(p.step == 8 && p.issued == 80);
  }
  {
    // grow target = grown_cap(bound + n): 2867 <= 2867.2 stays, 2868 doubles
    // until the need fills at most half (2868 <= 4096 = 8192 / 2)
    wh::LinearGuardPlan p;
    p.due(2800, cap, ml, false);  // bound 2800
    EXPECT(p.grow_target(67, cap, ml) == 4096);
    EXPECT(p.grow_target(68, cap, ml) == 8192);
    // "the exact count before growing": 2800 + 100 asks for 8192; the newest
    // summary then says that the 2800 ids were 900 keys, and 900 + 100 fits
    EXPECT(p.grow_target(100, cap, ml) == 8192);
    p.summarised(900, 2800);
    EXPECT(p.bound() == 900 && p.grow_target(100, cap, ml) == 4096);
    // and one that confirms the need keeps the target: 2790 + 100 > 2867.2
    p.summarised(2790, 2800);
    EXPECT(p.grow_target(100, cap, ml) == 8192);
  }
}

// the growers' histogram task lists (tasks x 5, red x 6) on literal vectors
static void test_gbdt_hist_plan() {
  using V = std::vector<int32_t>;
  using Groups = std::vector<std::pair<int64_t, int64_t>>;
  const Groups one{{0, 4}};
  auto plan = [](std::vector<int64_t> seglen, const Groups& fg, int chunk) {
    std::pair<V, V> p;
    wh::gbdt_hist_plan(seglen, fg, chunk, &p.first, &p.second);
    return p;
  };
  // one row, and an empty segment: one chunk each
  for (int64_t len : {1, 0}) {
    auto p = plan({len}, one, 4);
    EXPECT((p.first == V{0, 0, 4, 0, 4}));
    EXPECT((p.second == V{0, 0, 4, 0, 1, 1}));
  }
  // exactly a chunk stays one task; one row more makes two
  {
    auto p = plan({4}, one, 4);
    EXPECT((p.first == V{0, 0, 4, 0, 4}));
    EXPECT((p.second == V{0, 0, 4, 0, 1, 1}));
    p = plan({5}, one, 4);
    EXPECT((p.first == V{0, 0, 4, 0, 4, 0, 0, 4, 1, 4}));
    EXPECT((p.second == V{0, 0, 4, 0, 2, 1}));
  }
  // two segments (3 chunks and 1) of two feature groups: chunk-major tasks,
  // the second segment's tasks begin at t0 = 6
  {
    auto p = plan({9, 3}, Groups{{0, 4}, {4, 3}}, 4);
    EXPECT((p.first == V{0, 0, 4, 0, 4, 0, 4, 3, 0, 4, 0, 0, 4, 1, 4, 0, 4, 3, 1, 4,
                         0, 0, 4, 2, 4, 0, 4, 3, 2, 4, 1, 0, 4, 0, 4, 1, 4, 3, 0, 4}));
    EXPECT(p.first.size() / 5 == (3 + 1) * 2);
    EXPECT((p.second == V{0, 0, 4, 0, 3, 2, 0, 4, 3, 1, 3, 2, 1, 0, 4, 6, 1, 2, 1, 4, 3, 7, 1, 2}));
  }
  // the lists are appended to: t0 counts the tasks already there
  {
    auto p = plan({1}, one, 4);
    wh::gbdt_hist_plan({1}, one, 4, &p.first, &p.second);
    EXPECT((p.first == V{0, 0, 4, 0, 4, 0, 0, 4, 0, 4}));
    EXPECT((p.second == V{0, 0, 4, 0, 1, 1, 0, 0, 4, 1, 1, 1}));
  }
}

// the host grower's level tables: the segment tiling of [0, n) (expected
// values: the runs of models/gbdt.py _pos_node for the same segments) and the
// upload's word offsets
static void test_gbdt_level_plan() {
  using Tiles = std::vector<std::array<int, 2>>;  // {begin, node}
  using Segs = std::vector<std::array<int, 3>>;    // {begin, end, node}
  // no live segment: one gap over everything
  EXPECT((wh::gbdt_level_tiles(Segs{}, 10) == Tiles{{0, -1}}));
  // one segment covering [0, n)
  EXPECT((wh::gbdt_level_tiles(Segs{{0, 10, 0}}, 10) == Tiles{{0, 0}}));
  // gaps at the front, in the middle and at the end
  EXPECT((wh::gbdt_level_tiles(Segs{{2, 5, 3}, {7, 9, 4}}, 12) ==
          Tiles{{0, -1}, {2, 3}, {5, -1}, {7, 4}, {9, -1}}));
  EXPECT((wh::gbdt_level_tiles(Segs{{3, 10, 7}}, 10) == Tiles{{0, -1}, {3, 7}}));
  EXPECT((wh::gbdt_level_tiles(Segs{{0, 3, 7}}, 10) == Tiles{{0, 7}, {3, -1}}));
  // adjacent segments: no gap tile between them, in position order whatever
  // order they come in
  EXPECT((wh::gbdt_level_tiles(Segs{{0, 4, 1}, {4, 10, 2}}, 10) == Tiles{{0, 1}, {4, 2}}));
  EXPECT((wh::gbdt_level_tiles(Segs{{6, 10, 5}, {0, 6, 2}}, 10) == Tiles{{0, 2}, {6, 5}}));
  // word offsets: five nodes' defl bytes take two words
  {
    const wh::GbdtNodeTables at(/*nnode=*/5, /*nt=*/3, /*nsplit=*/2);
    EXPECT(at.feat == 0 && at.bin == 5 && at.sb == 10 && at.se == 15 && at.defl == 20);
    EXPECT(at.tb == 22 && at.tn == 25 && at.sp == 28 && at.par == 36);
    EXPECT(at.lc == 38 && at.rc == 43 && at.nwords == 48);
  }
  // a multiple of four leaves no padding; one node still takes a whole word
  EXPECT(wh::GbdtNodeTables(8, 1, 1).tb == 32 + 2);
  EXPECT(wh::GbdtNodeTables(1, 1, 0).tb == 4 + 1);
  EXPECT(wh::GbdtNodeTables(1, 1, 0).nwords == 5 + 1 + 1 + 0 + 0 + 1 + 1);
}

// the node weight and the children's constraints (host/gbdt_node_rule.h: the
// functions every grower and the kernels call)
static void test_gbdt_node_rule() {
  const double inf = std::numeric_limits<double>::infinity();
  auto same = [](const wh::GbdtBounds& a, double lo, double hi) { return a.lo == lo && a.hi == hi; };
  // the L1 threshold: at |G| = alpha, on either side of it, and without alpha
  EXPECT(wh::gbdt_l1(2.0, 2.0) == 0.0 && wh::gbdt_l1(-2.0, 2.0) == 0.0);
  EXPECT(wh::gbdt_l1(2.5, 2.0) == 0.5 && wh::gbdt_l1(-2.5, 2.0) == -0.5);
  EXPECT(wh::gbdt_l1(1.5, 2.0) == 0.0 && wh::gbdt_l1(-1.5, 2.0) == 0.0);
  EXPECT(wh::gbdt_l1(1.5, 0.0) == 1.5 && wh::gbdt_l1(-1.5, 0.0) == -1.5);
  EXPECT(std::signbit(wh::gbdt_l1(-0.0, 0.0)));
  // the weight: at H == mcw, just below it, and with lambda = 0
  EXPECT(wh::gbdt_weight0(3.0, 2.0, 0.0, 1.0, 2.0) == -1.0);
  EXPECT(wh::gbdt_weight0(3.0, std::nextafter(2.0, 0.0), 0.0, 1.0, 2.0) == 0.0);
  EXPECT(wh::gbdt_weight0(3.0, 2.0, 0.0, 0.0, 2.0) == -1.5);
  EXPECT(wh::gbdt_weight0(3.0, 2.0, 1.0, 0.0, 0.0) == -1.0);
  // weight intervals under monotone_constraints
  const wh::GbdtBounds root{-inf, inf}, b{-1.0, 2.0};
  EXPECT(wh::gbdt_clamp_weight(0.25, root) == 0.25);
  EXPECT(wh::gbdt_clamp_weight(-3.0, b) == -1.0 && wh::gbdt_clamp_weight(5.0, b) == 2.0);
  EXPECT(wh::gbdt_clamp_weight(2.0, b) == 2.0 && wh::gbdt_clamp_weight(-1.0, b) == -1.0);
  // a negative zero inside the interval stays what it is (leaf text "-0")
  EXPECT(std::signbit(wh::gbdt_clamp_weight(-0.0, wh::GbdtBounds{0.0, 1.0})));
  EXPECT(wh::gbdt_weight(3.0, 2.0, 0.0, 0.0, 2.0, b) == -1.0);
  auto up = wh::gbdt_child_bounds(1, root, -0.5, 1.5);
  EXPECT(same(up.left, -inf, 0.5) && same(up.right, 0.5, inf));
  auto down = wh::gbdt_child_bounds(-1, b, 1.0, 0.0);
  EXPECT(same(down.left, 0.5, 2.0) && same(down.right, -1.0, 0.5));
  auto free_ = wh::gbdt_child_bounds(0, b, 1.0, 0.0);
  EXPECT(same(free_.left, -1.0, 2.0) && same(free_.right, -1.0, 2.0));
  // a finite root (max_delta_step = 0.7 on either side of 0), children clamped to it
  const wh::GbdtBounds step{-0.7, 0.7};
  const double wl = wh::gbdt_clamp_weight(-3.0, step), wr = wh::gbdt_clamp_weight(0.25, step);
  const double mid = (-0.7 + 0.25) / 2;
  up = wh::gbdt_child_bounds(1, step, wl, wr);
  EXPECT(same(up.left, -0.7, mid) && same(up.right, mid, 0.7));
  down = wh::gbdt_child_bounds(-1, step, wl, wr);
  EXPECT(same(down.left, mid, 0.7) && same(down.right, -0.7, mid));
  free_ = wh::gbdt_child_bounds(0, step, wl, wr);
  EXPECT(same(free_.left, -0.7, 0.7) && same(free_.right, -0.7, 0.7));
  // group sets under interaction_constraints: an ungrouped feature (bit 63
  // alone) is admitted at the root only, and nothing below a split on it
  const uint64_t free_f = wh::kGbdtInterFree, g0 = 1, g1 = 2, g01 = 3;
  EXPECT(wh::gbdt_admits(wh::kGbdtInterRoot, free_f) && wh::gbdt_admits(wh::kGbdtInterRoot, g1));
  EXPECT(wh::gbdt_child_state(wh::kGbdtInterRoot, free_f) == 0);
  EXPECT(!wh::gbdt_admits(wh::gbdt_child_state(wh::kGbdtInterRoot, free_f), free_f));
  EXPECT(wh::gbdt_child_state(wh::kGbdtInterRoot, g01) == g01);
  EXPECT(!wh::gbdt_admits(g01, free_f) && wh::gbdt_admits(g01, g1));
  // disjoint groups: a split on one shuts the other out
  EXPECT(wh::gbdt_child_state(wh::kGbdtInterRoot, g0) == g0 && !wh::gbdt_admits(g0, g1));
  EXPECT(wh::gbdt_child_state(g0, g1) == 0 && wh::gbdt_child_state(g01, g1) == g1);
  // the shared weight against the host grower's former spelling (H < mcw
  // first, the threshold with an early return)
  auto old_l1 = [](double g, double alpha) {
    if (alpha <= 0) return g;
    return g > alpha ? g - alpha : (g < -alpha ? g + alpha : 0.0);
  };
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> ug(-8.0, 8.0), uh(0.0, 4.0);
  for (int i = 0; i < 400; ++i) {
    const double G = ug(rng), H = uh(rng), alpha = i % 3 ? uh(rng) : 0.0;
    const double lambda = i % 5 ? uh(rng) : 0.0, mcw = i % 7 ? uh(rng) : H;
    const double want = H < mcw ? 0.0 : -old_l1(G, alpha) / (H + lambda);
    const double got = wh::gbdt_weight0(G, H, alpha, lambda, mcw);
    EXPECT(std::memcmp(&got, &want, 8) == 0);
  }
}

// the objectives' gradient pairs and the metrics' row losses
// (host/gbdt_objective.h: the functions the kernels call) against their
// formulas in double, and the hinge table exactly
static void test_gbdt_objective() {
  const wh::GbdtObjScalars a = wh::gbdt_obj_scalars(0.7, 1.5, 2.0, 3.0);
  EXPECT(a.max_delta_step == 0.7f && a.tw1 == -0.5f && a.tw2 == 0.5f && a.delta2 == 4.f);
  auto near = [](float got, double want, double scale) {
    return std::fabs((double)got - want) <= 1e-6 * scale;
  };
  for (float m : {-4.f, -0.75f, 0.f, 0.5f, 3.25f})
    for (float y : {0.25f, 1.f, 3.f}) {
      const double M = m, Y = y, e = std::exp(M);
      auto p = wh::gbdt_obj_pair<wh::kObjPoisson>(m, y, a);
      EXPECT(near(p.g, e - Y, e + Y) && near(p.h, std::exp(M + 0.7), std::exp(M + 0.7)));
      p = wh::gbdt_obj_pair<wh::kObjGamma>(m, y, a);
      EXPECT(near(p.g, 1 - Y / e, 1 + Y / e) && near(p.h, Y / e, Y / e) && !p.scaled);
      p = wh::gbdt_obj_pair<wh::kObjTweedie>(m, y, a);
      const double e1 = std::exp(-0.5 * M), e2 = std::exp(0.5 * M);
      EXPECT(near(p.g, -Y * e1 + e2, Y * e1 + e2));
      EXPECT(near(p.h, 0.5 * Y * e1 + 0.5 * e2, 0.5 * Y * e1 + 0.5 * e2));
      p = wh::gbdt_obj_pair<wh::kObjPseudoHuber>(m, y, a);
      const double z = M - Y, s = std::sqrt(1 + z * z / 4);
      EXPECT(near(p.g, z / s, std::fabs(z / s)) && near(p.h, 1 / (s * s * s), 1.0));
      p = wh::gbdt_obj_pair<wh::kObjSquaredLog>(m, y, a);
      const double mm = std::max(M, (double)wh::kSquaredLogMinMargin);
      const double lm = std::log1p(mm), ly = std::log1p(Y), d = mm + 1;
      EXPECT(near(p.g, (lm - ly) / d, (std::fabs(lm) + std::fabs(ly)) / d));
      EXPECT(near(p.h, std::max((1 - lm + ly) / (d * d), 1e-6),
                  (1 + std::fabs(lm) + std::fabs(ly)) / (d * d)));
      p = wh::gbdt_obj_pair<wh::kObjLogistic>(m, y, a);
      const double q = 1 / (1 + std::exp(-M));
      EXPECT(near(p.g, q - Y, q + Y) && near(p.h, q * (1 - q), 1.0));
    }
  // hinge: (y, side of the margin) -> the pair; a satisfied row is final
  auto hinge = [&](float m, float y) { return wh::gbdt_obj_pair<wh::kObjHinge>(m, y, a); };
  EXPECT(hinge(0.5f, 1.f).g == -1.f && hinge(0.5f, 1.f).h == 1.f && !hinge(0.5f, 1.f).scaled);
  EXPECT(hinge(1.f, 1.f).g == 0.f && hinge(1.f, 1.f).h == FLT_MIN && hinge(1.f, 1.f).scaled);
  EXPECT(hinge(-0.5f, 0.f).g == 1.f && hinge(-0.5f, 0.f).h == 1.f);
  EXPECT(hinge(-1.5f, 0.f).g == 0.f && hinge(-1.5f, 0.f).h == FLT_MIN);
  // the adaptive objectives: h = 1 per unit weight; sign(0) = 0, d = 0 on the d >= 0 side
  auto mae = [&](float m, float y) { return wh::gbdt_obj_pair<wh::kObjAbsolute>(m, y, a); };
  EXPECT(mae(2.f, 1.f).g == 1.f && mae(0.f, 1.f).g == -1.f && mae(1.f, 1.f).g == 0.f);
  EXPECT(mae(2.f, 1.f).h == 1.f && !mae(2.f, 1.f).scaled);
  const auto aq = wh::gbdt_obj_scalars(0.0, 1.5, 1.0, 1.0, 0.125);
  auto pin = [&](float m, float y) { return wh::gbdt_obj_pair<wh::kObjQuantile>(m, y, aq); };
  EXPECT(pin(2.f, 1.f).g == 0.875f && pin(1.f, 1.f).g == 0.875f && pin(0.f, 1.f).g == -0.125f);
  EXPECT(pin(0.f, 1.f).h == 1.f && a.alpha == 0.5f);
  // scale_pos_weight multiplies the weight of the rows with y == 1 only
  EXPECT(wh::gbdt_obj_weight<wh::kObjLogistic>(2.f, 1.f, a) == 6.f);
  EXPECT(wh::gbdt_obj_weight<wh::kObjLogistic>(2.f, 0.f, a) == 2.f);
  EXPECT(wh::gbdt_obj_weight<wh::kObjPoisson>(2.f, 1.f, a) == 2.f);
  // links and row losses at round values
  EXPECT(wh::gbdt_link(wh::kLinkIdentity, -2.0) == -2.0 && wh::gbdt_link(wh::kLinkExp, 0.0) == 1.0);
  EXPECT(wh::gbdt_link(wh::kLinkSigmoid, 0.0) == 0.5);
  EXPECT(wh::gbdt_link(wh::kLinkStep, 0.0) == 0.0 && wh::gbdt_link(wh::kLinkStep, 0.1) == 1.0);
  auto loss = [](int k, double p, double y) { return wh::gbdt_metric_loss(k, p, y, 1.5, 2.0); };
  EXPECT(std::fabs(loss(wh::kMetPoissonNll, 1.0, 3.0) - (std::log(6.0) + 1.0)) < 1e-12);
  EXPECT(std::fabs(loss(wh::kMetPoissonNll, 0.0, 0.0) - 1e-16) < 1e-30);  // p clamped
  EXPECT(std::fabs(loss(wh::kMetGammaNll, 2.0, 3.0) - (1.5 + std::log(2.0))) < 1e-12);
  EXPECT(std::fabs(loss(wh::kMetGammaDeviance, 2.0, 2.0)) < 1e-12);
  EXPECT(std::fabs(loss(wh::kMetTweedieNll, 4.0, 3.0) - (3.0 * 0.5 * 2.0 + 2.0 * 2.0)) < 1e-12);
  EXPECT(loss(wh::kMetMae, 1.0, 3.5) == 2.5);
  EXPECT(std::fabs(loss(wh::kMetMphe, 1.0, 4.0) - 4.0 * (std::sqrt(1 + 9.0 / 4) - 1)) < 1e-12);
  EXPECT(std::fabs(loss(wh::kMetRmsle, 0.0, std::exp(1.0) - 1) - 1.0) < 1e-12);
}

// the localize job's bookkeeping (host/localize_plan.h) through the job
// sequences the GPU tests rely on. A Job mirrors what LocalizeJob holds.
static void test_localize_plan() {
  struct Job {
    int tab = -1;
    bool counted = false;
  };
  using Pool = wh::LocTablePool;
  // two jobs in flight and a third refused; slots alternate
  {
    Pool p;
    Job a, b;
    a.tab = p.acquire();
    b.tab = p.acquire();
    EXPECT(a.tab == 0 && b.tab == 1 && p.acquire() == -1);
    EXPECT(p.prepare(a.tab, 1024, 1024) == Pool::kReady);
    p.assigned(a.tab);
    EXPECT(!p.busy[0] && !p.dirty[0] && p.busy[1]);
    // `next` points at the held slot: the free one is taken instead
    EXPECT(p.next == 0);
    a.tab = p.acquire();
    EXPECT(a.tab == 0 && p.next == 1 && p.acquire() == -1);
    p.assigned(b.tab);
    p.assigned(a.tab);
    EXPECT(p.acquire() == 1 && p.acquire() == 0);
  }
  // abandon -> dirty -> refill before reuse; a clean slot needs nothing
  {
    Pool p;
    int t = p.acquire();
    EXPECT(p.prepare(t, 4096, 2048) == Pool::kReady && p.dirty[t]);
    p.abandoned(t);
    EXPECT(!p.busy[t] && p.dirty[t]);
    EXPECT(p.acquire() == 1);  // the other slot first
    p.assigned(1);
    EXPECT(p.acquire() == t);
    EXPECT(p.prepare(t, 4096, 2048) == Pool::kRefill);
    p.assigned(t);
    EXPECT(p.acquire() == 1);
    p.assigned(1);
    EXPECT(p.acquire() == t && p.prepare(t, 4096, 2048) == Pool::kReady);
  }
  // the hinted size overflows -> retry at the safe size on the same slot:
  // a table that is too small is reallocated, a large enough one refilled
  {
    const int64_t nnz = 100000, hint = 1000;
    const int64_t safe = wh::loc_safe_size(nnz), ts = wh::loc_hinted_size(hint, safe);
    EXPECT(safe == 262144 && ts == 4096);
    EXPECT(wh::loc_hinted_size(0, safe) == safe && wh::loc_hinted_size(safe, safe) == safe);
    EXPECT(wh::loc_safe_size(0) == 1024 && wh::loc_hinted_size(1, 1024) == 1024);
    Pool p;
    const int t = p.acquire();
    EXPECT(p.prepare(t, 1024, ts) == Pool::kRealloc);   // first use: 1024 entries
    EXPECT(p.prepare(t, safe, safe) == Pool::kRefill);  // (realloc is to the safe size)
    EXPECT(p.busy[t] && p.next == (t ^ 1));
    p.assigned(t);
    const int t2 = p.acquire(), t3 = p.acquire();
    EXPECT(t2 == (t ^ 1) && t3 == t && p.prepare(t3, safe, ts) == Pool::kReady);
    EXPECT(p.prepare(t3, safe, safe) == Pool::kRefill);
  }
  // the overflow decision: own flag at [nshard], the peers' at stride
  {
    const int64_t none[] = {5, 6, 0};
    auto o = wh::loc_overflow(none, 2, 0, 2);
    EXPECT(!o.own && !o.any);
    const int64_t own[] = {5, 6, 3};
    o = wh::loc_overflow(own, 2, 0, 2);
    EXPECT(o.own && o.any);
    // stride 3, world 2: {count, flag, extra} per peer; extras are not flags
    const int64_t peer[] = {5, 6, 0, 7, 0, 9, 8, 1, 9};
    o = wh::loc_overflow(peer, 2, 6, 3);
    EXPECT(!o.own && o.any);
    const int64_t extra[] = {5, 6, 0, 7, 0, 9, 8, 0, 9};
    o = wh::loc_overflow(extra, 2, 6, 3);
    EXPECT(!o.own && !o.any);
  }
  // a partition overflow -> fall back to the hash path: the in-flight count
  // is released once and never goes below zero, whichever of finish, retry
  // and destruction come, in any order
  {
    const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (const auto& ord : order) {
      wh::LocHeavyElection h;
      Pool p;
      Job j, other;
      h.begin(1, 4, other.counted);
      h.begin(1, 4, j.counted);
      EXPECT(h.inflight == 2 && j.counted);
      for (int step : ord) {
        if (step == 1 && j.tab < 0) j.tab = p.acquire();  // the retry takes a table
        h.release(j.counted);
        EXPECT(h.inflight == 1 && !j.counted);
      }
      h.release(other.counted);
      EXPECT(h.inflight == 0);
      h.release(other.counted);
      EXPECT(h.inflight == 0);
    }
  }
  // heavy hints: the first job elects but reads none; the next reads what it
  // elected; a layout change and a job begun while another is in flight read
  // none, and the latter elects none and leaves parity and layout alone
  {
    wh::LocHeavyElection h;
    Job a, b, c;
    auto k = h.begin(3, 2, a.counted);
    EXPECT(k.elect && k.read == 0 && k.write == 1 && k.nho_read == 0);
    h.release(a.counted);
    k = h.begin(3, 2, a.counted);
    EXPECT(k.elect && k.read == 1 && k.write == 0 && k.nho_read == 2);
    k = h.begin(3, 2, b.counted);  // a is in flight
    EXPECT(!k.elect && k.nho_read == 0 && h.parity == 0 && h.inflight == 2);
    h.release(a.counted);
    h.release(b.counted);
    k = h.begin(3, 2, c.counted);  // reads what a elected
    EXPECT(k.elect && k.read == 0 && k.write == 1 && k.nho_read == 2);
    h.release(c.counted);
    k = h.begin(4, 2, c.counted);  // another shard count
    EXPECT(k.elect && k.read == 1 && k.nho_read == 0 && h.layout == 4 * 65536 + 2);
    h.release(c.counted);
    k = h.begin(4, 3, c.counted);  // another heavy-owner count
    EXPECT(k.elect && k.nho_read == 0);
    h.release(c.counted);
    k = h.begin(4, 0, c.counted);  // a plan without heavy owners: counted all the same
    EXPECT(!k.elect && c.counted && h.inflight == 1 && h.layout == 4 * 65536 + 3);
    h.release(c.counted);
    k = h.begin(4, 3, c.counted);
    EXPECT(k.elect && k.nho_read == 3);
  }
  // the hint sequence of uneven minibatches (rows x 8 non-zeros; the caller
  // hints with the previous minibatch's unique count): scaled up when the
  // minibatch grew, never below the caller's hint, never above nnz
  {
    wh::LocHintScale s;
    int64_t hint = 0;
    const int64_t rows[] = {200000, 2000, 200000, 500, 150000, 3000, 200000};
    for (int64_t r : rows) {
      const int64_t nnz = r * 8, prev = s.last_nnz;
      const int64_t sc = s.scaled(hint, nnz);
      EXPECT(sc >= hint && sc <= std::max(nnz, hint));
      if (hint > 0 && nnz > prev) EXPECT(sc == std::min(nnz, hint * nnz / prev + 1));
      else EXPECT(sc == hint);
      EXPECT(wh::loc_uest(sc, nnz) <= nnz && wh::loc_uest(sc, nnz) >= std::min(sc, nnz));
      const int64_t u = nnz / 5 + 7;  // (any unique count)
      s.finished(nnz, u);
      hint = u;
    }
    EXPECT(s.scaled(hint + 1, 1 << 30) == hint + 1);  // not the last job's count: as given
    EXPECT(s.scaled(0, 1 << 30) == 0);
    EXPECT(wh::loc_uest(0, 777) == 777 && wh::loc_uest(100, 5000) == 1149);
    EXPECT(wh::loc_heavy_thr(1000) == 1024 && wh::loc_heavy_thr(4 << 20) == 4096);
  }
}

// what the multi-shard step puts on the wire (host/psx_plan.h). Expected
// values from the Python twin kv/psx.py: _QFilter.layout with H = ceil(2n /
// vs), Psx._upload, the row rules of Psx._c2 / _c3 and the tail slices of
// Psx._counts / _vcount_exchange.
static void test_psx_plan() {
  using R = wh::PsxRows;
  // filter layout: DiFacto nb=1 vs=8 (W=8, R=12), nb=3 vs=16 (W=16, R=52),
  // linear nb=2 (W=64)
  {
    auto L = wh::psx_qlayout(false, 8, 8, 12, {3, 0, 5}, {2, 0, 1}, {1, 0, 2});
    EXPECT((L.desc == R{0, 6, 8, 16, 0, 2, 24, 0, 0, 0, 4, 0, 24, 10, 16, 8, 4, 4}));
    EXPECT((L.rows == R{4, 0, 5}) && L.ext == 48);
    L = wh::psx_qlayout(false, 16, 16, 52, {0, 7}, {0, 4}, {0, 1});
    EXPECT((L.desc == R{0, 0, 0, 0, 0, 0, 0, 14, 16, 64, 0, 2}));
    EXPECT((L.rows == R{0, 6}) && L.ext == 80);
    L = wh::psx_qlayout(true, 0, 64, 132, {65, 0, 64, 1}, {}, {});
    EXPECT((L.desc == R{0, 0, 0, 65, 0, 0, 65, 0, 0, 0, 2, 0, 65, 0, 0, 64, 2, 0, 129, 0, 0, 1, 3, 0}));
    EXPECT((L.rows == R{2, 0, 1, 1}) && L.ext == 130);
  }
  // segment tables: P=3, vs=8, with the previous step's vrecv; without one
  // the last P words stay zero; linear (vs=0): no header rows
  const R send{3, 0, 5}, recv{2, 4, 0}, pv{1, 0, 2};
  {
    auto s = wh::psx_segs(send, recv, 8, false, &pv);
    EXPECT((s.Hw == R{1, 0, 2}) && (s.Ho == R{1, 1, 0}));
    EXPECT((s.table == R{0, 3, 3, 8, 0, 1, 1, 3, 0, 2, 6, 6, 0, 1, 2, 2, 1, 0, 2}));
    s = wh::psx_segs(send, recv, 8, false, nullptr);
    EXPECT((s.table == R{0, 3, 3, 8, 0, 1, 1, 3, 0, 2, 6, 6, 0, 1, 2, 2, 0, 0, 0}));
    s = wh::psx_segs(send, recv, 0, true, &pv);
    EXPECT((s.Hw == R{0, 0, 0}) && (s.Ho == R{0, 0, 0}));
    EXPECT((s.table == R{0, 3, 3, 8, 0, 0, 0, 0, 0, 2, 6, 6, 0, 0, 0, 0, 1, 0, 2}));
  }
  // rows per peer: C2 sends the owner side and receives the worker side, C3
  // the other way round (here: as each exchange would name them)
  {
    const R Hw{1, 0, 2}, Ho{1, 1, 0}, vown{2, 1, 0}, vrecv{1, 0, 2}, z{0, 0, 0};
    auto d = wh::psx_sides(false, send, recv, Hw, Ho, vown, vrecv);
    const R c2_send = d.owner, c2_recv = d.worker, c3_send = d.worker, c3_recv = d.owner;
    EXPECT((c2_send == R{3, 2, 0}) && (c2_recv == R{2, 0, 4}));
    EXPECT(c3_send == c2_recv && c3_recv == c2_send);
    auto l = wh::psx_sides(true, send, recv, z, z, z, z);
    EXPECT(l.owner == recv && l.worker == send);  // C2: send recv's rows, get send's; C3 swaps
  }
  // count payload, P=2: {recv, overflow, vrecv, has-data} per peer, then vown
  {
    const int64_t tail[10] = {11, 91, 13, 0, 21, 92, 23, 1, 31, 32};
    auto c = wh::psx_counts(tail, 2);
    EXPECT((c.recv == R{11, 21}) && (c.vrecv == R{13, 23}) && (c.vown == R{31, 32}) && c.any);
    const int64_t none[10] = {0, 1, 5, 0, 0, 0, 6, 0, 7, 8};
    c = wh::psx_counts(none, 2);
    EXPECT(!c.any && (c.vrecv == R{5, 6}) && (c.vown == R{7, 8}));  // "empty": no rank has data
    // the V-count exchange reads the same layout at offset S + 1 (S = 1)
    const int64_t buf[12] = {-1, -2, 11, 91, 13, 0, 21, 92, 23, 1, 31, 32};
    c = wh::psx_counts(buf + 1 + 1, 2);
    EXPECT((c.recv == R{11, 21}) && (c.vrecv == R{13, 23}) && (c.vown == R{31, 32}) && c.any);
  }
}

int main() {
  test_auc();
  test_auc_jobs();
  test_store_guard_plan();
  test_linear_guard_plan();
  test_localize_plan();
  test_psx_plan();
  test_gbdt_hist_plan();
  test_gbdt_level_plan();
  test_gbdt_node_rule();
  test_gbdt_objective();
  test_lz4();
  test_crb();
  test_parsers();
  test_splits_and_reader();
  test_conf();
  test_pool_concurrent();
  test_json();
  test_van();
  if (g_fail) {
    std::fprintf(stderr, "host_selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("host_selftest: ok\n");
  return 0;
}
