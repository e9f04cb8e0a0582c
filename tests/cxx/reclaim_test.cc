// FreeList and DeferredQueue (gandiva_amd/csrc/gdv_reclaim.h) without HIP: the deterministic contract of both, then eight
// threads over one queue and one token list with a ninth completing tokens in random order.  The tokens are fakes whose
// wait / release abort when they meet a state that only a SECOND owner of the same entry could have produced.  Built plain and
// with -fsanitize=thread by tests/test_reclaim_cpu.py; exit status 0 = every check held.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "gdv_reclaim.h"

using gdv::DeferredQueue;
using gdv::FreeList;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "reclaim_test.cc:%d: CHECK failed: %s\n", __LINE__, #cond); \
      std::abort();                                                                  \
    }                                                                                \
  } while (0)

namespace {

[[noreturn]] void Die(const char* what) {
  std::fprintf(stderr, "reclaim_test: %s\n", what);
  std::abort();
}

enum State : int { kIdle, kRecorded, kWaitedOn, kReleased, kDestroyed };

struct Token {
  std::atomic<int> state{kIdle};
  std::atomic<bool> complete{false};
};

void Record(Token* t) {
  t->complete.store(false);
  int was = kIdle;
  if (!t->state.compare_exchange_strong(was, kRecorded)) Die("record of a token that is not idle: it has another owner");
}
bool IsReady(Token* t) {  // what the queue calls under its lock: a query
  if (t->state.load() != kRecorded) Die("query of a queued token that somebody waits on or has released");
  return t->complete.load();
}
void Wait(Token* t) {
  int was = kRecorded;
  if (!t->state.compare_exchange_strong(was, kWaitedOn))
    Die(was == kWaitedOn ? "two threads wait on one token" : "wait on a released, idle or destroyed token");
  while (!t->complete.load()) std::this_thread::yield();
}
void Release(Token* t) {
  const int was = t->state.exchange(kReleased);
  if (was != kRecorded && was != kWaitedOn) Die("release of a token that is not in flight (double release)");
  if (!t->complete.load()) Die("release of a token that has not completed");
}

using Queue = DeferredQueue<Token*>;

// ------------------------------------------------------------------------------------------------ deterministic cases

void TestFreeList() {
  int destroyed = 0, last_destroyed = -1;
  FreeList<int> list(3, [&](int v) { destroyed++; last_destroyed = v; });
  int v = -1;
  CHECK(!list.Take(&v) && v == -1);          // empty
  for (int i = 1; i <= 3; i++) list.Give(i);  // up to the cap
  CHECK(destroyed == 0);
  list.Give(4);                               // one past the cap: destroyed, exactly once
  CHECK(destroyed == 1 && last_destroyed == 4);
  for (int want = 3; want >= 1; want--) CHECK(list.Take(&v) && v == want);  // last in first out
  CHECK(!list.Take(&v));
  CHECK(destroyed == 1);

  // the destroy function runs outside the lock: it may use the list it belongs to
  FreeList<int>* self = nullptr;
  int taken_inside = 0;
  FreeList<int> reentrant(1, [&](int) { int w = 0; if (self->Take(&w)) taken_inside = w; });
  self = &reentrant;
  reentrant.Give(7);
  reentrant.Give(8);
  CHECK(taken_inside == 7);
}

void TestQueue() {
  std::vector<std::unique_ptr<Token>> tokens;
  auto fresh = [&] { tokens.push_back(std::make_unique<Token>()); Record(tokens.back().get()); return tokens.back().get(); };
  std::vector<int> ran;

  {  // TakeReady: exactly the complete entries, in push order; the others stay queued in order
    Queue q;
    Token* t[6];
    for (int i = 0; i < 6; i++) { t[i] = fresh(); q.Push(t[i], 1, [&ran, i] { ran.push_back(i); }); }
    for (int i : {4, 1, 3}) t[i]->complete.store(true);
    auto ready = q.TakeReady(IsReady);
    CHECK(ready.size() == 3 && ready[0].token == t[1] && ready[1].token == t[3] && ready[2].token == t[4]);
    CHECK(ran.empty());  // the queue itself runs nothing
    for (auto& e : ready) { Release(e.token); e.done(); }
    CHECK((ran == std::vector<int>{1, 3, 4}));
    CHECK(q.TakeReady(IsReady).empty());
    auto rest = q.TakeAll();  // TakeAll empties the queue
    CHECK(rest.size() == 3 && rest[0].token == t[0] && rest[1].token == t[2] && rest[2].token == t[5]);
    CHECK(q.TakeAll().empty());
  }
  {  // TakeOldestIf counts one tag only
    Queue q;
    Queue::Entry e;
    e.tag = 99;
    CHECK(!q.TakeOldestIf(512, 8, &e) && e.tag == 99);  // empty queue
    Token* tagged[8];
    for (int i = 0; i < 27; i++) {  // 7 entries tagged 512 among 20 tagged 4096
      const bool mine = i % 4 == 1 && i / 4 < 7;
      Token* tk = fresh();
      if (mine) tagged[i / 4] = tk;
      q.Push(tk, mine ? 512 : 4096, [] {});
    }
    CHECK(!q.TakeOldestIf(512, 8, &e) && e.tag == 99);  // 7 of the tag, 20 of another: nothing
    tagged[7] = fresh();
    q.Push(tagged[7], 512, [] {});
    CHECK(q.TakeOldestIf(512, 8, &e) && e.token == tagged[0] && e.tag == 512);  // 8: the oldest of them
    CHECK(!q.TakeOldestIf(512, 8, &e));                                            // 7 remain ...
    auto rest = q.TakeAll();
    size_t left = 0;
    for (auto& r : rest)
      if (r.tag == 512) CHECK(r.token == tagged[++left]);  // ... in order
    CHECK(left == 7 && rest.size() == 27);
  }
  {  // a `done` may use the queue and a list: nothing runs under either lock
    Queue q;
    FreeList<Token*> list(4, [](Token*) {});
    Token* a = fresh();
    Token* b = fresh();
    int done_runs = 0;
    q.Push(a, 0, [&] {
      done_runs++;
      q.Push(b, 0, [&] { done_runs++; });
      list.Give(a);
    });
    for (auto& e : q.TakeAll()) e.done();
    for (auto& e : q.TakeAll()) e.done();
    Token* got = nullptr;
    CHECK(done_runs == 2 && list.Take(&got) && got == a && q.TakeAll().empty());
  }
}

// ------------------------------------------------------------------------------------------------ the concurrent case

constexpr int kThreads = 8, kRounds = 20000, kTags = 3, kCapPerTag = 8, kListCap = 16;

struct Shared {
  Queue queue;
  std::atomic<int> created{0}, destroyed{0};
  FreeList<Token*> idle{kListCap, [this](Token* t) {
    if (t->state.exchange(kDestroyed) != kReleased) Die("destroy of a token that was not released");
    destroyed++;
  }};
  std::mutex tokens_mu;
  std::vector<std::unique_ptr<Token>> tokens;   // every token ever made (destroyed ones stay allocated: their state is checked)
  std::mutex pending_mu;
  std::vector<Token*> pending;                  // recorded, not yet complete: what the completer draws from
  std::atomic<int> next_round{0};
  std::atomic<bool> workers_done{false};
  std::unique_ptr<std::atomic<int>[]> done_runs{new std::atomic<int>[kRounds]()};

  Token* Acquire() {
    Token* t = nullptr;
    if (idle.Take(&t)) {
      int was = kReleased;
      if (!t->state.compare_exchange_strong(was, kIdle)) Die("the list handed out a token that was not released");
      return t;
    }
    std::lock_guard<std::mutex> g(tokens_mu);
    tokens.push_back(std::make_unique<Token>());
    created++;
    return tokens.back().get();
  }
  // the caller took `e` out of the queue: it alone waits, releases and runs done
  void Complete(Queue::Entry& e, bool wait) {
    if (wait) Wait(e.token);
    Release(e.token);
    idle.Give(e.token);
    e.done();
  }
};

void Worker(Shared* s, unsigned seed) {
  std::minstd_rand rng(seed);
  for (;;) {
    const int r = s->next_round.fetch_add(1);
    if (r >= kRounds) return;
    Token* t = s->Acquire();
    Record(t);
    {
      std::lock_guard<std::mutex> g(s->pending_mu);
      s->pending.push_back(t);
    }
    const size_t tag = 256u << (r % kTags);
    std::atomic<int>* runs = &s->done_runs[r];
    s->queue.Push(t, tag, [runs] {
      if (runs->fetch_add(1) != 0) Die("a done ran twice");
    });
    const unsigned pick = static_cast<unsigned>(rng());
    if (pick % 64 == 0) {
      for (auto& e : s->queue.TakeAll()) s->Complete(e, true);
    } else {
      if (pick % 4 != 0)
        for (auto& e : s->queue.TakeReady(IsReady)) s->Complete(e, false);
      Queue::Entry oldest;
      if (s->queue.TakeOldestIf(tag, kCapPerTag, &oldest)) s->Complete(oldest, true);
    }
  }
}

void Completer(Shared* s) {
  std::minstd_rand rng(12345);
  for (;;) {
    Token* t = nullptr;
    {
      std::lock_guard<std::mutex> g(s->pending_mu);
      if (!s->pending.empty()) {
        const size_t i = static_cast<size_t>(rng()) % s->pending.size();
        t = s->pending[i];
        s->pending[i] = s->pending.back();
        s->pending.pop_back();
      } else if (s->workers_done.load()) {
        return;
      }
    }
    if (t != nullptr) t->complete.store(true);
    else std::this_thread::yield();
  }
}

void TestConcurrent() {
  Shared s;
  std::thread completer(Completer, &s);
  std::vector<std::thread> workers;
  for (int i = 0; i < kThreads; i++) workers.emplace_back(Worker, &s, 1000u + static_cast<unsigned>(i));
  for (auto& w : workers) w.join();
  for (auto& e : s.queue.TakeAll()) s.Complete(e, true);  // what the last rounds left queued
  s.workers_done.store(true);
  completer.join();

  CHECK(s.queue.TakeAll().empty());
  for (int r = 0; r < kRounds; r++) CHECK(s.done_runs[r].load() == 1);
  int idle = 0;
  Token* t = nullptr;
  while (s.idle.Take(&t)) {
    CHECK(t->state.load() == kReleased);
    idle++;
  }
  CHECK(idle <= kListCap && idle + s.destroyed.load() == s.created.load());
  for (auto& tk : s.tokens) CHECK(tk->state.load() == kReleased || tk->state.load() == kDestroyed);
  std::printf("reclaim_test: %d rounds on %d threads, %d tokens made, %d destroyed, %d idle at the end\n", kRounds, kThreads,
              s.created.load(), s.destroyed.load(), idle);
}

}  // namespace

int main() {
  TestFreeList();
  TestQueue();
  TestConcurrent();
  std::printf("reclaim_test: ok\n");
  return 0;
}
