// fdh_calllog.h -- the call recorder (fdh_record_begin / fdh_record_json): every BackendContext-level call between the two, as a JSON
// array of [name, args...].  One per context, written by the calling thread's recorder only (a pool thread's recorder has none).
#pragma once
#include <cstddef>
#include <string>

namespace fdh {

class CallLog {
 public:
  bool on() const { return on_; }
  void begin() { on_ = true; first_ = true; s_ = "["; }
  const char* json() {
    if (!on_) return "[]";
    s_ += "\n]";
    on_ = false;
    return s_.c_str();
  }
  // a call's entry, opened: its arguments and the closing bracket are the caller's (fdh_record.cpp: Rec).  Null while the log is off.
  std::string* open(const char* name) {
    if (!on_) return nullptr;
    mark_ = s_.size(); mark_first_ = first_;  // (a call that turns out to be culled is taken back: drop_last)
    s_ += first_ ? "[\"" : ",\n[\""; s_ += name; s_ += "\""; first_ = false;
    return &s_;
  }
  // cull mode 2 (culling while the log runs): the draw call just logged left no record -- it leaves no entry either
  void drop_last() { if (on_) { s_.resize(mark_); first_ = mark_first_; } }
  struct Pause {  // a backend method that calls other backend methods logs only itself
    // (writes the flag only where it was on -- i.e. on the calling thread while the call recorder runs, when nothing is handed to the walk
    // pool: written unconditionally, false over false, it was a data race between the pool's threads; ThreadSanitizer, profiles/r06_host_asan.txt)
    CallLog* const log;
    explicit Pause(CallLog* l) : log(l && l->on_ ? l : nullptr) { if (log) log->on_ = false; }
    ~Pause() { if (log) log->on_ = true; }
  };

 private:
  std::string s_;
  bool on_ = false, first_ = true, mark_first_ = true;
  size_t mark_ = 0;  // where the last entry begins
};

}  // namespace fdh
